"""GPU: the mixed-query top-k (vm_topk_cosine_mix, csrc/topk_mix.hip) against tests/mix_ref.py.

Bar: rows, fp64 score bits and padding identical to statement (A) of the oracle, for the fast and the ``exact=True``
entry.  The scan test runs the shapes at which the shared tile scan can go wrong (tests/tile_scan_data.py) for
every (C, J, weight set, mask set, k) of tests/mix_ref.py and demands flag 0 wherever the oracle's scores allow it: the
redo would hide a broken scan.  That they allow it is asserted from the oracle's scores before any search, and proven
without a GPU in tests/test_mix_cpu.py.
"""
import numpy as np
import pytest
import torch

from tests import mask_ref as MR
from tests import mix_ref as XR
from tests.search_checks import mix_check as check
from tests.search_checks import mix_want as want_of
from tests.support import bits, clustered, dev_mask, plain_memory, queries_near, redone, same_result, scan_memory
from tests.tile_scan_data import dataset

pytestmark = pytest.mark.gpu


# ---- 1. the scan ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(MR.SHAPES))
@pytest.mark.parametrize("D,dtype", XR.DTS)
def test_scan(D, dtype, shape):
    mem, q_all, base, live, total, cap = scan_memory(D, dtype, shape)
    n = live.shape[1]
    demanded = cases = 0
    for C in XR.CS:
        sels = XR.scan_selections(C, shape, base, n)
        sets = {"none": (None, None)}
        sets.update({name: (dev_mask(masks), index) for name, (masks, index) in MR.mask_sets(C, shape).items()})
        for J in XR.JS:
            terms = q_all[torch.tensor([XR.term_rows(c, J) for c in range(C)])].contiguous()      # [C, J, D]
            for wname in XR.WEIGHT_SETS:
                W, w = XR.scan_scores(D, dtype, shape, J, wname)                       # (A), from the shared matrix
                A = XR.abs_sum(w)
                for name, (masks, index) in sets.items():
                    sel = sels[name]
                    for k in XR.KS:
                        # the condition of the flag-0 demand, from oracle scores, before any search
                        ok = [XR.flag0_ok(np.sort(W[c][sel[c]])[::-1], k, D, A) for c in range(C)]
                        if name == "none":
                            assert all(ok), f"precondition: {shape} D={D} {dtype} J={J} {wname} k={k}"
                        want = MR.masked_topk_from_scores(W[:C], sel, k, base=base)
                        got_r, got_s, _ = check(mem, terms, w, k, dtype, masks, index, certified=ok, want=want,
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
    for k in (1, 10, 64):
        # J = 1, w = 1: the reference cosine bit for bit
        for exact in (False, True):
            got = mem.topk_mix(q[:, None, :], [1.0], k, exact=exact)
            assert same_result(got, mem.topk(q, k)), (k, exact)
            got = mem.topk_mix(q[:, None, :], [1.0], k, mask=mask, exact=exact)
            assert same_result(got, mem.topk_masked(q, k, mask)), (k, exact)
    # zero-weight padding from J = 3 to J = 16 changes no bit
    t3 = q[:15].reshape(5, 3, -1).contiguous()
    t16 = torch.cat([t3, q[None, :13].expand(5, -1, -1)], dim=1).contiguous()
    for w3 in ([1.0, 1.0, -0.5], [0.25, -2.0, 1.0 / 3]):
        for exact in (False, True):
            a = mem.topk_mix(t3, w3, 10, mask=mask, exact=exact)
            b = mem.topk_mix(t16, w3 + [0.0] * 13, 10, mask=mask, exact=exact)
            assert same_result(a, b), (w3, exact)
    # a query's result is the same alone and inside a batch of 3
    terms = q[:15].reshape(3, 5, -1).contiguous()
    ws = [XR.weights_of(nm, 5) for nm in ("mean", "feedback", "wide")]
    masks = torch.cat([mask, ~mask, mask])
    for exact in (False, True):
        s3, r3 = mem.topk_mix(terms, ws, 10, mask=masks, exact=exact)
        for c in range(3):
            s1, r1 = mem.topk_mix(terms[c], [ws[c]], 10, mask=masks[c], exact=exact)
            assert same_result((s1, r1), (s3[c:c + 1], r3[c:c + 1])), (c, exact)
    check(mem, terms, ws, 10, dtype, masks.cpu().numpy().view(np.uint32), label="batch of 3")
    mem.close()


# ---- 3. what must go to the redo and still be exact -------------------------------------------------------------------
def _redone(mem, terms, weights, k, dtype, label, flag=None, **kw):
    return redone(lambda: check(mem, terms, weights, k, dtype, label=label, **kw), lambda: mem.mix_uncertified_count,
                  terms.shape[0], label, flag)


def test_redo_cases():
    from vidmem import _lib
    rows, _ = clustered([5] * 8, 128, "f16", seed=31)
    mem = plain_memory(rows, "f16")
    q = queries_near(rows, 6, 4, "f16")
    terms = q.reshape(2, 3, -1).contiguous()
    # all weights 0: every W is 0.0, the first k live selected rows by id come back with score 0.0
    got_r, got_s = _redone(mem, terms, [0.0, 0.0, 0.0], 5, "f16", "all zero", flag=_lib.VM_FLAG_GAP)
    assert got_r.tolist() == [[0, 1, 2, 3, 4]] * 2 and (got_s == 0.0).all() and not np.signbit(got_s).any()
    mask = MR.pack_rows(range(3, 40, 2), 40)[None]
    got_r, _ = _redone(mem, terms, [0.0, 0.0, 0.0], 5, "f16", "all zero, masked", masks=mask)
    assert got_r.tolist() == [[3, 5, 7, 9, 11]] * 2
    # w = (1, -1) on two identical terms: the exact W is 0.0 for every row, whatever the fp32 scan made of it
    twice = torch.stack([q[:2], q[:2]], dim=1).contiguous()
    got_r, got_s = _redone(mem, twice, [1.0, -1.0], 5, "f16", "cancelling", flag=_lib.VM_FLAG_GAP)
    assert got_r.tolist() == [[0, 1, 2, 3, 4]] * 2 and (got_s == 0.0).all()
    # a weight outside the bound's domain
    got_r, _ = _redone(mem, terms, [2.0 ** 30, 1.0, -0.5], 5, "f16", "weight 2^30", flag=_lib.VM_FLAG_GAP)
    assert (got_r >= 0).all()
    _redone(mem, terms, [2.0 ** -30, 1.0, -0.5], 5, "f16", "weight 2^-30", flag=_lib.VM_FLAG_GAP)
    mem.close()
    # a static scene: 40 identical rows
    still = rows[7:8].expand(40, -1).contiguous()
    mem = plain_memory(still, "f16")
    got_r, _ = _redone(mem, terms, XR.weights_of("feedback", 3), 5, "f16", "static scene", flag=_lib.VM_FLAG_GAP)
    assert got_r.tolist() == [[0, 1, 2, 3, 4]] * 2
    mem.close()
    # a bf16 term whose norm is outside [2^-40, 2^40]
    rows, _ = clustered([5] * 8, 128, "bf16", seed=32)
    mem = plain_memory(rows, "bf16")
    q = queries_near(rows, 4, 4, "bf16")
    tiny = (q[2:4].float() * 2.0 ** -50).to(torch.bfloat16)
    assert float(tiny.double().norm(dim=1).max()) < 2.0 ** -40 and (tiny.float() != 0).any()
    terms = torch.stack([q[:2], tiny], dim=1).contiguous()
    _redone(mem, terms, [1.0, 0.5], 5, "bf16", "tiny bf16 term", flag=_lib.VM_FLAG_GAP)
    mem.close()


# ---- 4. ring and lifecycle ----------------------------------------------------------------------------------------------
def test_ring_after_overwrites_erase_and_device_built_exclusion():
    D, dtype = 128, "f16"
    rows, q_all, base, _ = dataset(D, dtype, "ring40")
    more, _ = clustered([4] * 6, D, dtype, seed=41)
    mem = plain_memory(rows, dtype, capacity=40, ring=True, step=19)
    terms = q_all[:15].reshape(3, 5, -1).contiguous()
    ws = [XR.weights_of(nm, 5) for nm in ("mean", "feedback", "wide")]
    check(mem, terms, ws, 5, dtype, label="ring")
    mem.append(more[:13])                                           # overwrites 13 more rows: the seam moves
    assert mem.rows_host()[0] == base + 13
    got_r, _, _ = check(mem, terms, ws, 5, dtype, label="ring after appends")
    assert (got_r >= base + 13).all()
    check(mem, terms, ws, 5, dtype, MR.pack_rows(range(base + 13, base + 53, 2), 40)[None], label="ring, masked")
    mem.close()
    # a linear memory after an erase
    rows, _ = clustered([5] * 12, D, dtype, seed=42)
    mem = plain_memory(rows, dtype, capacity=64)
    check(mem, terms, ws, 5, dtype, label="before erase")
    mem.erase(rows=[0, 7, 8, 9, 30, 59])
    assert len(mem) == 54
    check(mem, terms, ws, 5, dtype, label="after erase")
    # the mask built on the device from a previous search: the hits of round one are excluded from round two
    s1, r1 = mem.topk(terms[:, 0].contiguous(), 5)
    shown = mem.mask_of_rows(r1)
    got_r, _, _ = check(mem, terms, ws, 5, dtype, (~shown).cpu().numpy().view(np.uint32)[None], label="exclusion")
    assert not set(got_r.ravel().tolist()) & set(r1.cpu().numpy().ravel().tolist())
    s2, r2 = mem.topk_mix(terms, ws, 5, mask=~shown)
    assert np.array_equal(r2.cpu().numpy(), got_r)
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
    for cut in (0.3, 0.0, -0.2, None):                              # a strict filter on the raw sum, negative included
        got_r, got_s, _ = check(mem, terms, ws, 64, "bf16", masks, [2, 0, 1], min_score=cut, label=f"min_score {cut}")
        if cut is not None:
            assert (got_s[got_r >= 0] > cut).all() and (got_r == -1).any()
        if cut is not None and cut < 0:
            assert (got_s[got_r >= 0] < 0).any()                    # scores below zero pass a negative threshold
    check(mem, terms, ws, 64, "bf16", min_score=-0.2, label="negative threshold, unmasked")
    got_r, _, _ = check(mem, terms, ws, 5, "bf16", masks, [0, 3, -1], label="index out of range")
    assert (got_r[1:] == -1).all() and (got_r[0] >= 0).all()
    plain = check(mem, terms, ws, 7, "bf16", label="stride 1")
    base, host_rows = mem.rows_host()
    wr, wscore = XR.mix_topk(bits(terms), ws, host_rows, None, 7, dtype="bf16")
    for exact in (False, True):
        s, r = mem.topk_mix(terms, ws, 7, stride=(3, 1), exact=exact)
        assert np.array_equal(r.cpu().numpy(), wr * 3 + 1) and np.array_equal(s.cpu().numpy().view(np.int64), wscore.view(np.int64))
    assert np.array_equal(plain[0], wr)
    # the C entry point refuses, with a text
    sc = mem.prepare_topk_mix(3, 4, 5)
    need = mem.L.vm_topk_mix_workspace_bytes(mem.handle, 3, 5)
    assert sc.ws.numel() >= need > 4 * 3 * 300
    w = torch.tensor(ws, dtype=torch.float64, device="cuda")
    out_s = torch.empty((3, 64), dtype=torch.float64, device="cuda")
    out_r = torch.empty((3, 64), dtype=torch.int64, device="cuda")
    m = dev_mask(masks)

    def call(J=4, k=5, outs=(out_s, out_r), ws_bytes=None, mask_ptr=None, n_masks=0, exact=False):
        head = (mem.handle, terms.data_ptr(), w.data_ptr(), 3, J, k, mask_ptr, n_masks, None, 0, 0.0, 1, 0,
                outs[0].data_ptr() if outs[0] is not None else None, outs[1].data_ptr() if outs[1] is not None else None)
        tail = (sc.ws.data_ptr(), sc.ws.numel() if ws_bytes is None else ws_bytes, _lib.current_stream_ptr())
        if exact:
            return mem.L.vm_topk_cosine_mix_exact(*head, *tail)
        return mem.L.vm_topk_cosine_mix(*head, None, None, *tail)

    for exact in (False, True):
        assert call(exact=exact) == _lib.VM_OK
        for kw, text in ((dict(J=0), "J=0"), (dict(J=17), "J=17"), (dict(k=0), "k=0"), (dict(k=65), "k=65"),
                         (dict(outs=(None, out_r)), "null outputs"), (dict(outs=(out_s, None)), "null outputs"),
                         (dict(ws_bytes=need - 1), "workspace"), (dict(mask_ptr=m.data_ptr() + 2, n_masks=3), "aligned"),
                         (dict(mask_ptr=m.data_ptr(), n_masks=2), "mask_index"),
                         (dict(mask_ptr=m.data_ptr(), n_masks=0), "mask_index")):
            assert call(exact=exact, **kw) == _lib.VM_ERR_INVALID, (kw, exact)
            assert text in mem.L.vm_last_error(mem.ctx.handle).decode(), (kw, mem.L.vm_last_error(mem.ctx.handle))
    torch.cuda.synchronize()
    mem.close()


def test_an_empty_memory():
    from vidmem.memory import EmbeddingMemory
    mem = EmbeddingMemory(64, 128, "f16")
    terms = torch.randn(2, 3, 128, device="cuda", generator=torch.Generator("cuda").manual_seed(3)).to(torch.float16)
    for exact in (False, True):
        for mask in (None, ~mem.new_mask()):
            s, r = mem.topk_mix(terms, [1.0, 0.5, -0.5], 4, mask=mask, exact=exact)
            assert (r == -1).all() and (s == 0.0).all()
    assert (mem.last_mix_flags[:2] == 0).all() and mem.mix_uncertified_count == 0
    mem.close()


# ---- 6. capture ---------------------------------------------------------------------------------------------------------
def test_graph_capture_replayed_after_an_append_and_rewritten_weights_and_mask():
    from vidmem.memory import EmbeddingMemory, MixTopkScratch
    rows, _ = clustered([4] * 128, 384, "f16", seed=61)
    mem = EmbeddingMemory(1024, 384, "f16")
    mem.append(rows[:256])
    C, J, k = 3, 4, 10
    mem.prepare_topk_mix(C, J, k)                     # the memory's counter exists before the capture
    scratch = MixTopkScratch.for_(mem, C, k)          # and the capture runs on a scratch the caller owns
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
            out_s, out_r = mem.topk_mix(terms, weights, k, mask=mask, mask_index=index, scratch=scratch)
    torch.cuda.current_stream().wait_stream(s)
    assert mem._own[MixTopkScratch] is not scratch and mem._last[MixTopkScratch] is scratch

    def replay_and_check(words, ws, label):
        mask.copy_(dev_mask(words))                   # rewritten in place
        weights.copy_(torch.tensor(ws, dtype=torch.float64))
        graph.replay()
        torch.cuda.synchronize()
        want_r, want_s = want_of(mem, terms, ws, k, "f16", words, [0, 1, 0])
        assert np.array_equal(out_r.cpu().numpy(), want_r), label
        assert np.array_equal(out_s.cpu().numpy().view(np.int64), want_s.view(np.int64)), label
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
