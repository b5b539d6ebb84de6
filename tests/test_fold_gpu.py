"""GPU: the any/all top-k (vm_topk_cosine_fold, csrc/topk_mix.hip) against tests/fold_ref.py.

Bar: rows, fp64 score bits, the winning term T and padding identical to statement (A) of the oracle, for the fast and the
``exact=True`` entry and both ops.  The scan test runs the shapes at which the shared tile scan can go wrong
(tests/tile_scan_data.py) for every (op, C, J, weight set, mask set, k) of tests/fold_ref.py and demands flag 0
wherever the oracle's scores allow it: the redo would hide a broken scan.  That they allow it is asserted from the
oracle's scores before any search, and proven without a GPU in tests/test_fold_cpu.py.
"""
import numpy as np
import pytest
import torch

from tests import fold_ref as FR
from tests import mask_ref as MR
from tests.search_checks import fold_check as check
from tests.search_checks import fold_want as want_of
from tests.support import bits, clustered, dev_mask, plain_memory, queries_near, redone, same_result, scan_memory
from tests.tile_scan_data import dataset

pytestmark = pytest.mark.gpu


# ---- 1. the scan ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", FR.OPS)
@pytest.mark.parametrize("shape", list(MR.SHAPES))
@pytest.mark.parametrize("D,dtype", FR.DTS)
def test_scan(D, dtype, shape, op):
    mem, q_all, base, live, total, cap = scan_memory(D, dtype, shape)
    n = live.shape[1]
    demanded = cases = 0
    for C in FR.CS:
        sels = FR.scan_selections(C, shape, base, n)
        sets = {"none": (None, None)}
        sets.update({name: (dev_mask(masks), index) for name, (masks, index) in MR.mask_sets(C, shape).items()})
        for J in FR.JS:
            terms = q_all[torch.tensor([FR.term_rows(c, J) for c in range(C)])].contiguous()      # [C, J, D]
            for wname in FR.WEIGHT_SETS:
                F, T, w = FR.scan_scores(D, dtype, shape, J, wname, op)                # (A), from the shared matrix
                A = FR.abs_max(w)
                for name, (masks, index) in sets.items():
                    sel = sels[name]
                    for k in FR.KS:
                        # the condition of the flag-0 demand, from oracle scores, before any search
                        ok = [FR.flag0_ok(np.sort(F[c][sel[c]])[::-1], k, D, A) for c in range(C)]
                        if name == "none":
                            assert all(ok), f"precondition: {shape} D={D} {dtype} {op} J={J} {wname} k={k}"
                        want_r, want_s = MR.masked_topk_from_scores(F[:C], sel, k, base=base)
                        want = (want_r, want_s, FR.terms_of_rows(T[:C], want_r, base))
                        got_r, got_s, _ = check(mem, terms, w, k, op, dtype, masks, index, certified=ok, want=want,
                                                label=f"{shape} C={C} J={J} {wname} {name} k={k}")
                        demanded += sum(ok)
                        cases += C
                        if name in ("empty", "first_dead"):
                            assert (got_r == -1).all() and (got_s == 0.0).all()
                        if name == "newest":
                            assert (got_r[:, 0] == total - 1).all() and (got_r[:, 1:] == -1).all()
    assert demanded >= 0.9 * cases
    mem.close()


# ---- 2. identities on the device --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_identities(dtype):
    rows, _ = clustered([5] * 200, 384, dtype, seed=21)
    mem = plain_memory(rows, dtype)
    q = queries_near(rows, 16, 9, dtype)
    mask = dev_mask(MR.pack_rows(range(100, 900, 3), mem.capacity)[None])
    for op in FR.OPS:
        for k in (1, 10, 64):
            # J = 1, w = 1: the reference cosine bit for bit
            for exact in (False, True):
                got = mem.topk_fold(q[:, None, :], k, op=op, exact=exact)
                assert same_result(got, mem.topk(q, k)), (op, k, exact)
                assert (got[2][got[1] >= 0] == 0).all()
                got = mem.topk_fold(q[:, None, :], k, op=op, mask=mask, exact=exact)
                assert same_result(got, mem.topk_masked(q, k, mask)), (op, k, exact)
            t = q[:15].reshape(3, 5, -1).contiguous()
            w = [1.0, 0.5, -0.5, 2.0, 1.0]
            perm = [3, 0, 4, 2, 1]
            for exact in (False, True):
                a = mem.topk_fold(t, k, op=op, weights=w, mask=mask, exact=exact)
                # permuting the terms with their weights changes no score bit and no row, only T
                b = mem.topk_fold(t[:, perm].contiguous(), k, op=op, weights=[w[i] for i in perm], mask=mask, exact=exact)
                assert same_result(a, b), (op, k, exact)
                assert (a[1] >= 0).all() and torch.equal(torch.tensor(perm, device="cuda")[b[2].long()].int(), a[2])
                # appending a copy of a term with its weight changes nothing at all
                d = mem.topk_fold(torch.cat([t, t[:, 1:2]], dim=1).contiguous(), k, op=op, weights=w + [w[1]], mask=mask,
                                  exact=exact)
                assert same_result(a, d) and torch.equal(a[2], d[2]), (op, k, exact)
        # a query's result is the same alone and inside a batch of 3
        terms = q[:15].reshape(3, 5, -1).contiguous()
        ws = [FR.weights_of(nm, 5) for nm in FR.WEIGHT_SETS]
        masks = torch.cat([mask, ~mask, mask])
        for exact in (False, True):
            s3, r3, t3 = mem.topk_fold(terms, 10, op=op, weights=ws, mask=masks, exact=exact)
            for c in range(3):
                s1, r1, t1 = mem.topk_fold(terms[c], 10, op=op, weights=[ws[c]], mask=masks[c], exact=exact)
                assert same_result((s1, r1), (s3[c:c + 1], r3[c:c + 1])) and torch.equal(t1, t3[c:c + 1]), (op, c, exact)
        check(mem, terms, ws, 10, op, dtype, masks.cpu().numpy().view(np.uint32), label="batch of 3")
    # max with unit weights against the J plain searches: the best fold score is the best of the J best cosines
    s, r, t = mem.topk_any(q[:5][None].contiguous(), 1)
    s5, r5 = mem.topk(q[:5], 1)
    assert float(s[0, 0]) == float(s5.max()) and int(r[0, 0]) in r5[:, 0].tolist()
    mem.close()


# ---- 3. what must go to the redo and still be exact -------------------------------------------------------------------
def _redone(mem, terms, weights, k, op, dtype, label, flag=None, **kw):
    return redone(lambda: check(mem, terms, weights, k, op, dtype, label=label, **kw), lambda: mem.fold_uncertified_count,
                  terms.shape[0], label, flag)


@pytest.mark.parametrize("op", FR.OPS)
def test_redo_cases(op):
    from vidmem import _lib
    rows, _ = clustered([5] * 8, 128, "f16", seed=31)
    mem = plain_memory(rows, "f16")
    q = queries_near(rows, 6, 4, "f16")
    terms = q.reshape(2, 3, -1).contiguous()
    # all weights 0: every product is +-0.0, the first k live selected rows by id come back
    got_r, got_s = _redone(mem, terms, [0.0, 0.0, 0.0], 5, op, "f16", "all zero", flag=_lib.VM_FLAG_GAP)
    assert got_r.tolist() == [[0, 1, 2, 3, 4]] * 2 and (got_s == 0.0).all()
    mask = MR.pack_rows(range(3, 40, 2), 40)[None]
    got_r, _ = _redone(mem, terms, [0.0, 0.0, 0.0], 5, op, "f16", "all zero, masked", masks=mask)
    assert got_r.tolist() == [[3, 5, 7, 9, 11]] * 2
    # two identical terms: every row ties between them and the first one wins T.  Unlike the mixed search's cancelling
    # pair this forces no redo: F is the cosine of the one term, and the oracle's scores say the query must be certified
    # (rank 5 and rank 14 lie more than 4 eps_fold apart) - so the flag is 0 and the counter stands still
    from oracle import cref
    twice = torch.stack([q[:2], q[:2]], dim=1).contiguous()
    F = cref.cosine_matrix(bits(q[:2]), mem.rows_host()[1], dtype="f16")
    ok = [FR.flag0_ok(np.sort(F[c])[::-1], 5, 128, 1.0) for c in range(2)]
    assert all(ok), "precondition: identical terms"
    before = mem.fold_uncertified_count
    _, _, flags = check(mem, twice, [1.0, 1.0], 5, op, "f16", certified=ok, label="identical terms")
    assert (flags == _lib.VM_FLAG_CERTIFIED).all() and mem.fold_uncertified_count == before
    s, r, t = mem.topk_fold(twice, 5, op=op)
    assert (t == 0).all() and (r >= 0).all()
    # weights outside the bound's domain
    got_r, _ = _redone(mem, terms, [2.0 ** 30, 1.0, -0.5], 5, op, "f16", "weight 2^30", flag=_lib.VM_FLAG_GAP)
    assert (got_r >= 0).all()
    _redone(mem, terms, [2.0 ** -30, 1.0, -0.5], 5, op, "f16", "weight 2^-30", flag=_lib.VM_FLAG_GAP)
    mem.close()
    # a static scene: 40 identical rows
    still = rows[7:8].expand(40, -1).contiguous()
    mem = plain_memory(still, "f16")
    got_r, _ = _redone(mem, terms, FR.weights_of("signed", 3), 5, op, "f16", "static scene", flag=_lib.VM_FLAG_GAP)
    assert got_r.tolist() == [[0, 1, 2, 3, 4]] * 2
    mem.close()
    # a bf16 term whose norm is outside [2^-40, 2^40]
    rows, _ = clustered([5] * 8, 128, "bf16", seed=32)
    mem = plain_memory(rows, "bf16")
    q = queries_near(rows, 4, 4, "bf16")
    tiny = (q[2:4].float() * 2.0 ** -50).to(torch.bfloat16)
    assert float(tiny.double().norm(dim=1).max()) < 2.0 ** -40 and (tiny.float() != 0).any()
    terms = torch.stack([q[:2], tiny], dim=1).contiguous()
    _redone(mem, terms, [1.0, 0.5], 5, op, "bf16", "tiny bf16 term", flag=_lib.VM_FLAG_GAP)
    mem.close()


def test_certificate_uses_the_largest_weight():
    """Sixteen copies of one term with unit weights: A = max |w_j| = 1, their sum is 16.  Rank 1 and rank M + 1 are more
    than 4 eps_fold(D, 1) apart, so the query must be certified; with the sum as A the certificate would ask for a gap
    of eps_fold(D, 16) and leave it to the redo (tests/test_fold_cpu.py, defect 8)."""
    row_bits, term, gap = FR.certificate_gap_case()
    D = row_bits.shape[1]
    assert 4 * FR.eps_fold(D, 1.0) < gap <= FR.eps_fold(D, 16.0) - FR.eps_fold(D, 1.0)
    rows = torch.from_numpy(row_bits.view(np.int16)).view(torch.float16).cuda()
    mem = plain_memory(rows, "f16")
    terms = rows[0].expand(1, 16, -1).contiguous()
    for op in FR.OPS:
        got_r, got_s, flags = check(mem, terms, [1.0] * 16, 1, op, "f16", certified=[True], label="largest weight")
        assert got_r.tolist() == [[0]] and got_s.tolist() == [[1.0]] and flags.tolist() == [0]
    assert mem.fold_uncertified_count == 0
    mem.close()


# ---- 4. ring and lifecycle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", FR.OPS)
def test_ring_after_overwrites_erase_and_device_built_exclusion(op):
    D, dtype = 128, "f16"
    rows, q_all, base, _ = dataset(D, dtype, "ring40")
    more, _ = clustered([4] * 6, D, dtype, seed=41)
    mem = plain_memory(rows, dtype, capacity=40, ring=True, step=19)
    terms = q_all[:15].reshape(3, 5, -1).contiguous()
    ws = [FR.weights_of(nm, 5) for nm in FR.WEIGHT_SETS]
    check(mem, terms, ws, 5, op, dtype, label="ring")
    mem.append(more[:13])                                           # overwrites 13 more rows: the seam moves
    assert mem.rows_host()[0] == base + 13
    got_r, _, _ = check(mem, terms, ws, 5, op, dtype, label="ring after appends")
    assert (got_r >= base + 13).all()
    check(mem, terms, ws, 5, op, dtype, MR.pack_rows(range(base + 13, base + 53, 2), 40)[None], label="ring, masked")
    mem.close()
    # a linear memory after an erase
    rows, _ = clustered([5] * 12, D, dtype, seed=42)
    mem = plain_memory(rows, dtype, capacity=64)
    check(mem, terms, ws, 5, op, dtype, label="before erase")
    mem.erase(rows=[0, 7, 8, 9, 30, 59])
    assert len(mem) == 54
    check(mem, terms, ws, 5, op, dtype, label="after erase")
    # the mask built on the device from a previous search: the hits of round one are excluded from round two
    s1, r1 = mem.topk(terms[:, 0].contiguous(), 5)
    shown = mem.mask_of_rows(r1)
    got_r, _, _ = check(mem, terms, ws, 5, op, dtype, (~shown).cpu().numpy().view(np.uint32)[None], label="exclusion")
    assert not set(got_r.ravel().tolist()) & set(r1.cpu().numpy().ravel().tolist())
    mem.close()


# ---- 5. arguments -------------------------------------------------------------------------------------------------------
def test_arguments():
    from vidmem import _lib
    rows, _ = clustered([5] * 60, 384, "bf16", seed=51)
    mem = plain_memory(rows, "bf16", grouped=True)                  # any memory: here a grouped one
    q = queries_near(rows, 12, 5, "bf16")
    terms = q.reshape(3, 4, -1).contiguous()
    ws = [[1.0, 0.5, -0.5, 0.25], [0.5, 0.5, 0.5, 0.5], [1.0, -1.0, 1.0, -0.25]]
    rng = np.random.default_rng(1)
    masks = np.stack([MR.pack_rows(np.nonzero(rng.random(300) < p)[0], 300) for p in (0.5, 0.1, 0.03)])
    for op in FR.OPS:
        for cut in (0.3, 0.0, -0.2, None):                          # a strict filter on the raw value
            got_r, got_s, _ = check(mem, terms, ws, 64, op, "bf16", masks, [2, 0, 1], min_score=cut, label=f"min_score {cut}")
            if cut is not None:
                assert (got_s[got_r >= 0] > cut).all() and (got_r == -1).any()
        got_r, _, _ = check(mem, terms, ws, 5, op, "bf16", masks, [0, 3, -1], label="index out of range")
        assert (got_r[1:] == -1).all() and (got_r[0] >= 0).all()
        plain = check(mem, terms, ws, 7, op, "bf16", label="stride 1")
        base, host_rows = mem.rows_host()
        wr, wscore, wt = FR.fold_topk(bits(terms), ws, host_rows, None, 7, op, dtype="bf16")
        for exact in (False, True):
            s, r, t = mem.topk_fold(terms, 7, op=op, weights=ws, stride=(3, 1), exact=exact)
            assert np.array_equal(r.cpu().numpy(), wr * 3 + 1) and np.array_equal(t.cpu().numpy(), wt)
            assert np.array_equal(s.cpu().numpy().view(np.int64), wscore.view(np.int64))
        assert np.array_equal(plain[0], wr)
    # the C entry point refuses, with a text, and writes nothing
    sc = mem.prepare_topk_fold(3, 4, 5)
    need = mem.L.vm_topk_fold_workspace_bytes(mem.handle, 3, 5)
    assert sc.ws.numel() >= need > 4 * 3 * 300 and need == mem.L.vm_topk_mix_workspace_bytes(mem.handle, 3, 5)
    w = torch.tensor(ws, dtype=torch.float64, device="cuda")
    out_s = torch.full((3, 64), 7.0, dtype=torch.float64, device="cuda")
    out_r = torch.full((3, 64), 7, dtype=torch.int64, device="cuda")
    out_t = torch.full((3, 64), 7, dtype=torch.int32, device="cuda")
    m = dev_mask(masks)

    def call(J=4, k=5, op=0, outs=(out_s, out_r), ws_bytes=None, mask_ptr=None, n_masks=0, exact=False, stride=1, C=3):
        head = (mem.handle, terms.data_ptr(), w.data_ptr(), C, J, k, op, mask_ptr, n_masks, None, 0, 0.0, stride, 0,
                outs[0].data_ptr() if outs[0] is not None else None, outs[1].data_ptr() if outs[1] is not None else None,
                out_t.data_ptr())
        tail = (sc.ws.data_ptr(), sc.ws.numel() if ws_bytes is None else ws_bytes, _lib.current_stream_ptr())
        if exact:
            return mem.L.vm_topk_cosine_fold_exact(*head, *tail)
        return mem.L.vm_topk_cosine_fold(*head, None, None, *tail)

    for exact in (False, True):
        for kw, text in ((dict(J=0), "J=0"), (dict(J=17), "J=17"), (dict(k=0), "k=0"), (dict(k=65), "k=65"),
                         (dict(op=2), "vm_fold_op"), (dict(op=-1), "vm_fold_op"), (dict(op=3), "vm_fold_op"),
                         (dict(C=0), "C=0"), (dict(stride=0), "row_stride"),
                         (dict(outs=(None, out_r)), "null outputs"), (dict(outs=(out_s, None)), "null outputs"),
                         (dict(ws_bytes=need - 1), "workspace"), (dict(mask_ptr=m.data_ptr() + 2, n_masks=3), "aligned"),
                         (dict(mask_ptr=m.data_ptr(), n_masks=2), "mask_index"),
                         (dict(mask_ptr=m.data_ptr(), n_masks=0), "mask_index")):
            assert call(exact=exact, **kw) == _lib.VM_ERR_INVALID, (kw, exact)
            assert text in mem.L.vm_last_error(mem.ctx.handle).decode(), (kw, mem.L.vm_last_error(mem.ctx.handle))
        torch.cuda.synchronize()
        assert (out_s == 7.0).all() and (out_r == 7).all() and (out_t == 7).all()      # every refusal wrote nothing
    for exact in (False, True):
        for op in (0, 1):
            assert call(exact=exact, op=op) == _lib.VM_OK
    torch.cuda.synchronize()
    assert (out_r.view(-1)[:15] != 7).all() and (out_t.view(-1)[:15] != 7).all()
    mem.close()


def test_an_empty_memory():
    from vidmem.memory import EmbeddingMemory
    mem = EmbeddingMemory(64, 128, "f16")
    terms = torch.randn(2, 3, 128, device="cuda", generator=torch.Generator("cuda").manual_seed(3)).to(torch.float16)
    for op in FR.OPS:
        for exact in (False, True):
            for mask in (None, ~mem.new_mask()):
                s, r, t = mem.topk_fold(terms, 4, op=op, weights=[1.0, 0.5, -0.5], mask=mask, exact=exact)
                assert (r == -1).all() and (s == 0.0).all() and (t == -1).all()
    assert (mem.last_fold_flags[:2] == 0).all() and mem.fold_uncertified_count == 0
    mem.close()


# ---- 6. capture ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", FR.OPS)
def test_graph_capture_replayed_after_an_append_and_rewritten_weights_and_mask(op):
    from vidmem.memory import EmbeddingMemory, FoldTopkScratch
    rows, _ = clustered([4] * 128, 384, "f16", seed=61)
    mem = EmbeddingMemory(1024, 384, "f16")
    mem.append(rows[:256])
    C, J, k = 3, 4, 10
    mem.prepare_topk_fold(C, J, k)                    # the memory's counter exists before the capture
    scratch = FoldTopkScratch.for_(mem, C, k)         # and the capture runs on a scratch the caller owns
    terms = queries_near(rows, C * J, 6, "f16").reshape(C, J, -1).contiguous()
    weights = torch.tensor([[1.0, 0.5, 0.25, -0.5]] * C, dtype=torch.float64, device="cuda")
    mask = mem.new_mask(2)
    index = torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):       # one linear graph
            out_s, out_r, out_t = mem.topk_fold(terms, k, op=op, weights=weights, mask=mask, mask_index=index,
                                                scratch=scratch)
    torch.cuda.current_stream().wait_stream(s)
    assert mem._own[FoldTopkScratch] is not scratch and mem._last[FoldTopkScratch] is scratch

    def replay_and_check(words, ws, label):
        mask.copy_(dev_mask(words))                   # rewritten in place
        weights.copy_(torch.tensor(ws, dtype=torch.float64))
        graph.replay()
        torch.cuda.synchronize()
        want_r, want_s, want_t = want_of(mem, terms, ws, k, op, "f16", words, [0, 1, 0])
        assert np.array_equal(out_r.cpu().numpy(), want_r), label
        assert np.array_equal(out_s.cpu().numpy().view(np.int64), want_s.view(np.int64)), label
        assert np.array_equal(out_t.cpu().numpy(), want_t), label
        return want_r

    w0 = [[1.0, 0.5, 0.25, -0.5]] * C
    r = replay_and_check(np.stack([MR.pack_rows(range(0, 128), 1024), MR.pack_rows(range(100, 256), 1024)]), w0, "first")
    assert (r[0] < 128).all() and (r[1] >= 100).all()
    w1 = [[-1.0, 0.0, 2.0, 0.125], [0.0, 0.0, 0.0, 1.0], [0.25, 0.25, 0.25, 0.25]]
    r = replay_and_check(np.stack([MR.pack_rows(range(200, 400), 1024), MR.pack_rows([7], 1024)]), w1, "rewritten")
    assert ((r[0] >= 200) & (r[0] < 256)).all() and r[1].tolist() == [7] + [-1] * 9      # rows 256 .. 399 are not live yet
    mem.append(rows[256:512])
    terms.copy_(rows[300:312].reshape(C, J, -1))
    r = replay_and_check(np.stack([MR.pack_rows(range(200, 400), 1024), MR.pack_rows(range(0, 512, 2), 1024)]), w0, "appended")
    assert (r[0] >= 256).any() and (r[1] % 2 == 0).all()                                  # the rows appended since
    mem.close()


# ---- 7. the adapters ----------------------------------------------------------------------------------------------------
def test_linked_similarities_against_the_reference_merge():
    from oracle import cref
    from vidmem.similarity import batch_similarities, fold_similarities, linked_similarities, merge_batch_similarities
    rows, _ = clustered([3] * 40, 128, "f16", seed=71)
    mem = plain_memory(rows, "f16")
    mem.ids = [f"chunk-{i}" for i in range(len(mem))]
    ids = list(mem.ids)
    q = queries_near(rows, 40, 8, "f16")
    cos = cref.cosine_matrix(bits(q), bits(rows), dtype="f16")
    mask = dev_mask(MR.pack_rows(range(0, 120, 2), mem.capacity)[None])
    sel = MR.selected(MR.pack_rows(range(0, 120, 2), mem.capacity), 0, 120, mem.capacity)
    for Q, k_each, k_final in ((1, 5, 5), (3, 10, 4), (7, 10, 10), (16, 10, 10), (17, 8, 8), (40, 10, 3)):
        emb = [q[i] for i in range(Q)]
        for msk, sl in ((None, None), (mask, sel)):
            want = FR.reference_linking(list(cos[:Q]), ids, k_each, k_final, sl)
            got = linked_similarities(mem, emb, k_each, k_final, mask=msk)
            assert [s for _, s in got] == [s for _, s in want], (Q, k_each, k_final)
            if len(set(s for _, s in want)) == len(want):
                assert got == want, (Q, k_each, k_final)
            assert want == merge_batch_similarities(batch_similarities(mem, emb, k_each, mask=msk), k_final)
    # failed entries contribute nothing
    emb = [q[0], ValueError("embedder failed"), q[1], None, q[2]]
    want = FR.reference_linking([cos[0], None, cos[1], None, cos[2]], ids, 6, 6)
    assert linked_similarities(mem, emb, 6, 6) == want
    assert linked_similarities(mem, [None, ValueError("x")], 6, 6) == []
    # the fallback branches are the two-step path itself: top_k_final > top_k_each, and a wrong-length embedding
    emb = [q[i] for i in range(4)]
    assert linked_similarities(mem, emb, 3, 6) == merge_batch_similarities(batch_similarities(mem, emb, 3), 6)
    short = [q[0], q[1][:64]]
    assert linked_similarities(mem, short, 5, 5) == merge_batch_similarities(batch_similarities(mem, short, 5), 5)
    # fold_similarities: the list shape of the fold itself
    t = q[:6].reshape(2, 3, -1).contiguous()
    for op in FR.OPS:
        wr, wscore, _ = FR.fold_topk(bits(t), [[1.0, 0.5, 2.0]] * 2, bits(rows), None, 4, op)
        got = fold_similarities(mem, t, 4, op=op, weights=[1.0, 0.5, 2.0])
        assert got == [[(ids[r], float(s)) for r, s in zip(rr, ss)] for rr, ss in zip(wr, wscore)]
    mem.close()
