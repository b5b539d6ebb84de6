"""GPU: the diverse top-k (vm_topk_cosine_diverse, csrc/topk_diverse.hip) against tests/diverse_ref.py.

Bar: rows, fp64 relevance bits, fp64 mmr bits and padding identical to statement (A) of the oracle, for the fast and the
``exact=True`` entry.  There is no tolerance: the contract fixes every rounding.  The scan test runs the shapes at which
the shared tile scan can go wrong (tests/tile_scan_data.py) and demands flag 0 wherever the oracle's scores
allow it - without a mask, everywhere: the redo would hide a broken scan.  That they allow it, and that the picks differ
from plain top-k at all, is proven without a GPU in tests/test_diverse_cpu.py.
"""
import numpy as np
import pytest
import torch

from tests import diverse_ref as DR
from tests import mask_ref as MR
from tests.support import bits, check_entries, clustered, dev_mask, plain_memory, queries_near, same_result, scan_memory
from tests.tile_scan_data import dataset

pytestmark = pytest.mark.gpu


def want_of(mem, q, k, pool, lam, dtype, masks=None, index=None, **kw):
    """Statement (A) for the memory as it is: q [Q,D] on the device, masks / index host arrays."""
    base, host_rows = mem.rows_host()
    sel = None if masks is None else MR.selection(masks, index, q.shape[0], base, host_rows.shape[0], mem.capacity)
    sim = DR.sim_matrix(host_rows, dtype) if host_rows.shape[0] <= 128 else None    # else pool by pool
    return DR.diverse_topk(bits(q), host_rows, sel, k, pool, lam, dtype=dtype, base=base, sim=sim, **kw)


def check(mem, q, k, pool, lam, dtype, masks=None, index=None, certified=None, label="", want=None, lam_dev=None, **kw):
    """Fast and exact entry against (A) (``want``: (A) computed by the caller).  certified: None, or bool per query - the
    pool stage must have answered those queries itself (flag 0).  lam_dev: the device tensor to pass in place of lam."""
    Q = q.shape[0]
    want = want or want_of(mem, q, k, pool, lam, dtype, masks, index, **kw)
    assert all(w.shape == (Q, k) for w in want), f"{label}: the oracle's outputs are not [Q, k]"
    m = None if masks is None else (masks if isinstance(masks, torch.Tensor) else dev_mask(masks))

    def call(exact):
        s, r = mem.topk_diverse(q, k, pool=pool, lam=lam if lam_dev is None else lam_dev, mask=m, mask_index=index,
                                exact=exact, **kw)
        return r, s, mem.last_diverse_mmr
    return check_entries(call, lambda: mem.last_diverse_flags[:Q], want, certified, label)


# ---- 1. the scan ------------------------------------------------------------------------------------------------------
class _Oracle:
    """(A) for the scan test's data, one query at a time and each (query, selection, k, pool, lam) once: the pool of a
    selection comes from one cref.cosine_topk call for all 33 queries, the pairs from one cref.cosine_matrix call."""

    def __init__(self, D, dtype, shape):
        self.rows, self.q, self.base, self.live = MR.host_case(D, dtype, shape)
        self.dtype = dtype
        self.sim = DR.sim_matrix(self.rows, dtype)
        self.pools, self.picks = {}, {}

    def _pool(self, sel_i, pool):
        key = (sel_i.tobytes(), pool)
        if key not in self.pools:
            sel = np.broadcast_to(sel_i, (self.q.shape[0], sel_i.size))
            self.pools[key] = MR.masked_topk(self.q, self.rows, sel, pool, dtype=self.dtype, base=self.base)
        return self.pools[key]

    def want(self, sel, k, pool, lams):
        Q = sel.shape[0]
        out = (np.full((Q, k), -1, np.int64), np.zeros((Q, k)), np.zeros((Q, k)))
        for i in range(Q):
            key = (i, sel[i].tobytes(), k, pool, lams[i])
            if key not in self.picks:
                pr, ps = self._pool(sel[i], pool)
                self.picks[key] = DR._pick_all(pr[i:i + 1], ps[i:i + 1], self.rows, k, lams[i], self.dtype, self.base,
                                               DR.greedy_loop, self.sim)
            for o, w in zip(out, self.picks[key]):
                o[i] = w[0]
        return out


@pytest.mark.parametrize("shape", list(MR.SHAPES))
@pytest.mark.parametrize("D,dtype", DR.DTS)
def test_scan(D, dtype, shape):
    mem, q_all, base, live, total, cap = scan_memory(D, dtype, shape)
    rows = dataset(D, dtype, shape)[0]
    ora = _Oracle(D, dtype, shape)
    assert ora.base == base and np.array_equal(bits(rows[base:]), ora.rows) and np.array_equal(bits(q_all), ora.q)
    n = live.shape[1]
    differ = 0
    for Q in DR.QS:
        q = q_all[:Q].contiguous()
        sets = {name: (None if masks is None else dev_mask(masks), index, sel)
                for name, (masks, index, sel) in DR.scan_selections(Q, shape, base, n).items()}
        for k, pool in DR.K_POOL:
            for name, (masks, index, sel) in sets.items():
                # the condition of the flag-0 demand, from oracle scores, before any search
                ok = [DR.flag0_ok(np.sort(live[i][sel[i]])[::-1], pool, D) for i in range(Q)]
                if name == "none":
                    assert all(ok), f"precondition (i): {shape} D={D} {dtype} pool={pool}"
                for lam in (*DR.LAMS, DR.lam_vector(Q)):
                    lams = DR.per_query(lam, Q)
                    got_r, got_s, got_v, _ = check(mem, q, k, pool, lam, dtype, masks, index, certified=ok,
                                                   want=ora.want(sel, k, pool, lams),
                                                   label=f"{shape} Q={Q} k={k} pool={pool} lam={lam} {name}")
                    if name in ("empty", "first_dead"):
                        assert (got_r == -1).all() and (got_s == 0.0).all() and (got_v == 0.0).all()
                    if name == "none" and Q == 33 and (k, pool) == (5, 16) and lam == 0.5:
                        plain = ora.want(sel, k, pool, [1.0] * Q)[0]
                        differ = int((got_r != plain).any(axis=1).sum())
    assert 2 * differ >= 33, f"the picks equal plain top-5 for all but {differ} of 33 queries"
    mem.close()


# ---- 2. identities on the device --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_identities(dtype):
    rows, _ = clustered([5] * 200, 384, dtype, seed=21)
    mem = plain_memory(rows, dtype)
    q = queries_near(rows, 33, 9, dtype)
    mask = dev_mask(MR.pack_rows(range(100, 900, 3), mem.capacity)[None])
    for k in (1, 10, 64):
        # lam = 1: the rows and scores of topk / topk_masked, whatever the pool
        for exact in (False, True):
            for pool in (k, 64):
                got = mem.topk_diverse(q, k, pool=pool, lam=1.0, exact=exact)
                assert same_result(got, mem.topk(q, k)), (k, pool, exact)
                assert np.array_equal(mem.last_diverse_mmr.cpu().numpy().view(np.int64),
                                      got[0].cpu().numpy().view(np.int64))             # 1.0 e - 0.0 red = e
                got = mem.topk_diverse(q, k, pool=pool, lam=1.0, mask=mask, exact=exact)
                assert same_result(got, mem.topk_masked(q, k, mask)), (k, pool, exact)
    # a query's result is the same alone and inside a batch of 33
    lam = DR.lam_vector(33)
    masks = torch.cat([mask, ~mask])
    index = [i % 2 for i in range(33)]
    for exact in (False, True):
        s33, r33 = mem.topk_diverse(q, 10, pool=40, lam=lam, mask=masks, mask_index=index, exact=exact)
        v33 = mem.last_diverse_mmr.clone()
        for c in (0, 15, 16, 32):
            s1, r1 = mem.topk_diverse(q[c], 10, pool=40, lam=lam[c], mask=masks[index[c]], exact=exact)
            assert same_result((s1, r1), (s33[c:c + 1], r33[c:c + 1])), (c, exact)
            assert torch.equal(mem.last_diverse_mmr.view(torch.int64), v33[c:c + 1].view(torch.int64))
    check(mem, q, 10, 40, lam, dtype, masks.cpu().numpy().view(np.uint32), index, label="batch of 33")
    # pool == k only reorders the top k
    s, r = mem.topk_diverse(q, 10, pool=10, lam=0.3)
    assert torch.equal(r.sort(dim=1).values, mem.topk(q, 10)[1].sort(dim=1).values)
    mem.close()


# ---- 3. what must go to the redo and still be exact -------------------------------------------------------------------
def _duplicates_case():
    """100 fp16 rows: 8 distinct views of the query with orthogonal rests (ids 0 .. 7), 52 copies of one background row
    (8 .. 59), 40 exact copies of the query (60 .. 99).  At pool 64, ranks 49 .. 100 tie exactly, so rank 64 cannot clear
    rank M + 1 = 81: the pool stage must flag the query."""
    g = torch.Generator(device="cpu").manual_seed(71)
    D = 128
    basis = torch.linalg.qr(torch.randn(D, 10, generator=g, dtype=torch.float64)).Q.T      # 10 orthonormal rows
    qv = basis[0]
    views = 0.6 * qv + 0.8 * basis[1:9]
    background = 0.1 * qv + (1 - 0.01) ** 0.5 * basis[9]
    rows = torch.cat([views, background.expand(52, -1), qv.expand(40, -1)]).to(torch.float16)
    return rows.cuda(), qv.to(torch.float16)[None].cuda()


def test_redo_cases():
    from vidmem import _lib
    rows, q = _duplicates_case()
    mem = plain_memory(rows, "f16")
    before = mem.diverse_uncertified_count
    got_r, got_s, got_v, flags = check(mem, q, 5, 64, 0.5, "f16", label="40 duplicates of the query")
    assert flags[0] in (_lib.VM_FLAG_GAP, _lib.VM_FLAG_OVERFLOW) and mem.diverse_uncertified_count == before + 1
    assert got_r[0, 0] == 60 and int((got_r[0] >= 60).sum()) == 1          # the best row, then no copy of it
    plain = mem.topk(q, 5)[1].cpu().numpy()
    assert (plain >= 60).all()                                             # where plain top-k returns five copies
    check(mem, q, 40, 64, 0.0, "f16", label="40 duplicates, lam 0")
    # a zero query: every e is 0.0, the pool is the first rows by id
    zero = torch.zeros_like(q)
    got_r, got_s, _, _ = check(mem, zero, 5, 16, 0.5, "f16", label="zero query")
    assert set(got_r[0].tolist()) <= set(range(16)) and got_r[0, 0] == 0 and (got_s == 0.0).all()
    mem.close()
    # a zero stored row inside the pool: sim 0.0 with every row, e 0.0
    rows, _ = clustered([3] * 6, 128, "bf16", seed=72)
    rows[4] = 0
    mem = plain_memory(rows, "bf16")
    qs = queries_near(rows, 3, 5, "bf16")
    for pool in (18, 64):
        got_r, got_s, _, _ = check(mem, qs, pool if pool == 18 else 18, pool, 0.5, "bf16", label=f"zero row, pool {pool}")
        assert (got_r == 4).sum() == 3 and (got_s[got_r == 4] == 0.0).all()
    mem.close()


# ---- 4. shapes, arguments, memories --------------------------------------------------------------------------------------
def test_largest_row_tile_in_lds():
    rows, _ = clustered([4] * 25, 2048, "f16", seed=81)
    mem = plain_memory(rows, "f16")
    q = queries_near(rows, 3, 2, "f16")
    got_r, _, _, _ = check(mem, q, 20, 64, 0.5, "f16", label="D=2048")
    assert (got_r >= 0).all()
    mem.close()


def test_stride_min_score_and_an_empty_memory():
    rows, _ = clustered([5] * 60, 384, "bf16", seed=51)
    mem = plain_memory(rows, "bf16")
    q = queries_near(rows, 12, 5, "bf16")
    lam = DR.lam_vector(12)
    want = want_of(mem, q, 7, 30, lam, "bf16")
    for exact in (False, True):
        s, r = mem.topk_diverse(q, 7, pool=30, lam=lam, stride=(3, 1), exact=exact)
        assert np.array_equal(r.cpu().numpy(), want[0] * 3 + 1)
        assert np.array_equal(s.cpu().numpy().view(np.int64), want[1].view(np.int64))
        assert np.array_equal(mem.last_diverse_mmr.cpu().numpy().view(np.int64), want[2].view(np.int64))
    rng = np.random.default_rng(1)
    masks = np.stack([MR.pack_rows(np.nonzero(rng.random(300) < p)[0], 300) for p in (0.5, 0.1)])
    index = [i % 2 for i in range(12)]
    for cut in (0.3, 0.0, -0.2):                                    # a strict filter on the raw cosine
        got_r, got_s, _, _ = check(mem, q, 10, 40, lam, "bf16", min_score=cut, label=f"min_score {cut}")
        assert (got_s[got_r >= 0] > cut).all()
        if cut == 0.3:                                              # only the query's own cluster of 5 passes: fewer than k
            assert ((got_r >= 0).sum(axis=1) == 5).all() and (got_r[:, 5:] == -1).all()
        check(mem, q, 10, 40, lam, "bf16", masks, index, min_score=cut, label=f"min_score {cut}, masked")
    got_r, _, _, _ = check(mem, q, 10, 40, lam, "bf16", min_score=2.0, label="nothing passes")
    assert (got_r == -1).all()
    mem.close()
    from vidmem.memory import EmbeddingMemory
    mem = EmbeddingMemory(64, 128, "f16")
    qe = torch.randn(2, 128, device="cuda", generator=torch.Generator("cuda").manual_seed(3)).to(torch.float16)
    for exact in (False, True):
        for mask in (None, ~mem.new_mask()):
            s, r = mem.topk_diverse(qe, 4, mask=mask, exact=exact)
            assert (r == -1).all() and (s == 0.0).all() and (mem.last_diverse_mmr == 0.0).all()
    assert (mem.last_diverse_flags[:2] == 0).all() and mem.diverse_uncertified_count == 0
    mem.close()


def test_the_c_entry_refuses_with_a_text_and_leaves_the_outputs():
    from vidmem import _lib
    rows, _ = clustered([5] * 60, 384, "bf16", seed=51)
    mem = plain_memory(rows, "bf16")
    q = queries_near(rows, 3, 5, "bf16")
    sc = mem.prepare_topk_diverse(3, 5, 16)
    need = mem.L.vm_topk_diverse_workspace_bytes(mem.handle, 3, 16)
    assert sc.ws.numel() >= need > mem.L.vm_topk_masked_workspace_bytes(mem.handle, 3, 16) + 3 * 64 * 64 * 8
    for bad in ((0, 16), (3, 0), (3, 65), (1 << 21, 16)):
        assert mem.L.vm_topk_diverse_workspace_bytes(mem.handle, *bad) == 0
    lam = torch.full((3,), 0.5, dtype=torch.float64, device="cuda")
    outs = [torch.full((3, 64), 7.0, dtype=torch.float64, device="cuda"),
            torch.full((3, 64), 7, dtype=torch.int64, device="cuda"),
            torch.full((3, 64), 7.0, dtype=torch.float64, device="cuda")]
    m = mem.new_mask(3)

    def call(k=5, pool=16, Q=3, qp=q.data_ptr(), lp=lam.data_ptr(), outs=outs, ws_bytes=None, mask_ptr=None, n_masks=0,
             stride=1, exact=False):
        head = (mem.handle, qp, Q, k, pool, lp, mask_ptr, n_masks, None, 0, 0.0, stride, 0,
                *(o.data_ptr() if o is not None else None for o in outs))
        tail = (sc.ws.data_ptr(), sc.ws.numel() if ws_bytes is None else ws_bytes, _lib.current_stream_ptr())
        if exact:
            return mem.L.vm_topk_cosine_diverse_exact(*head, *tail)
        return mem.L.vm_topk_cosine_diverse(*head, None, None, *tail)

    INVALID, NOMEM = _lib.VM_ERR_INVALID, _lib.VM_ERR_NOMEM
    for exact in (False, True):
        for kw, code, text in ((dict(k=0), INVALID, "k=0"), (dict(k=65, pool=64), INVALID, "k=65"),
                               (dict(pool=0), INVALID, "pool=0"), (dict(pool=65), INVALID, "pool=65"),
                               (dict(k=9, pool=8), INVALID, "k=9 > pool=8"), (dict(Q=0), INVALID, "Q=0"),
                               (dict(qp=None), INVALID, "null queries or lam"), (dict(lp=None), INVALID, "null queries or lam"),
                               (dict(outs=[None, outs[1], outs[2]]), INVALID, "null outputs"),
                               (dict(outs=[outs[0], None, outs[2]]), INVALID, "null outputs"),
                               (dict(outs=[outs[0], outs[1], None]), INVALID, "null outputs"),
                               (dict(stride=0), INVALID, "row_stride"),
                               (dict(mask_ptr=m.data_ptr() + 2, n_masks=3), INVALID, "aligned"),
                               (dict(mask_ptr=m.data_ptr(), n_masks=2), INVALID, "mask_index"),
                               (dict(mask_ptr=m.data_ptr(), n_masks=0), INVALID, "mask_index"),
                               (dict(qp=q.data_ptr() + 2), INVALID, "aligned"),
                               (dict(ws_bytes=need - 1), NOMEM, "workspace"), (dict(ws_bytes=0), NOMEM, "workspace")):
            assert call(exact=exact, **kw) == code, (kw, exact)
            assert text in mem.L.vm_last_error(mem.ctx.handle).decode(), (kw, mem.L.vm_last_error(mem.ctx.handle))
    torch.cuda.synchronize()
    assert all((o == 7).all() for o in outs)                        # refused before any launch
    for exact in (False, True):
        assert call(exact=exact) == _lib.VM_OK
    torch.cuda.synchronize()
    want = want_of(mem, q, 5, 16, 0.5, "bf16")
    assert np.array_equal(outs[1].view(-1)[:15].view(3, 5).cpu().numpy(), want[0])
    mem.close()


@pytest.mark.parametrize("kind", ["plain", "grouped", "tagged", "ring", "erased"])
def test_any_memory(kind):
    D, dtype = 128, "f16"
    rows, _ = clustered([5] * 24, D, dtype, seed=91)
    q = queries_near(rows, 5, 8, dtype)
    lam = [0.5, 0.0, 1.0, 0.7, 0.3]
    if kind == "ring":
        mem = plain_memory(rows, dtype, capacity=70, ring=True, step=33)
        assert mem.rows_host()[0] == 50
    elif kind == "erased":
        mem = plain_memory(rows, dtype, capacity=128)
        mem.erase(rows=[0, 7, 8, 9, 30, 59, 119])
        mem.sync()
        assert len(mem) == 113
    else:
        mem = plain_memory(rows, dtype, **({} if kind == "plain" else {kind: True}))
    got_r, _, _, _ = check(mem, q, 8, 32, lam, dtype, label=kind)
    assert (got_r >= 0).all()
    base, host_rows = mem.rows_host()
    mask = MR.pack_rows(range(base, base + host_rows.shape[0], 2), mem.capacity)[None]
    got_r, _, _, _ = check(mem, q, 8, 32, lam, dtype, mask, label=f"{kind}, masked")
    assert ((got_r - base) % 2 == 0).all()
    mem.close()


# ---- 5. capture ---------------------------------------------------------------------------------------------------------
def test_graph_capture_of_append_and_search_replayed_with_rewritten_operands():
    from vidmem.memory import DiverseTopkScratch, EmbeddingMemory
    rows, _ = clustered([4] * 128, 384, "f16", seed=61)
    mem = EmbeddingMemory(1024, 384, "f16")
    mem.append(rows[:256])
    Q, k, pool = 3, 6, 24
    mem.prepare_topk_diverse(Q, k, pool)              # the memory's counter exists before the capture
    scratch = DiverseTopkScratch.for_(mem, Q, pool)   # and the capture runs on a scratch the caller owns
    q = queries_near(rows, Q, 6, "f16").contiguous()
    lam = torch.tensor([0.5, 0.5, 0.5], dtype=torch.float64, device="cuda")
    mask = mem.new_mask(2)
    index = torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda")
    src = rows[256:320].clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):       # one linear graph
            mem.append(src)
            out_s, out_r = mem.topk_diverse(q, k, pool=pool, lam=lam, mask=mask, mask_index=index, scratch=scratch)
    torch.cuda.current_stream().wait_stream(s)
    mem.sync()                                        # the capture advanced only the host mirror
    assert len(mem) == 256
    assert mem._own[DiverseTopkScratch] is not scratch and mem._last[DiverseTopkScratch] is scratch

    def replay_and_check(words, lams, label):
        mask.copy_(dev_mask(words))                   # rewritten in place
        lam.copy_(torch.tensor(lams, dtype=torch.float64))
        graph.replay()
        torch.cuda.synchronize()
        mem.sync()
        want_r, want_s, want_v = want_of(mem, q, k, pool, lams, "f16", words, [0, 1, 0])
        assert np.array_equal(out_r.cpu().numpy(), want_r), label
        assert np.array_equal(out_s.cpu().numpy().view(np.int64), want_s.view(np.int64)), label
        assert np.array_equal(mem.last_diverse_mmr.cpu().numpy().view(np.int64), want_v.view(np.int64)), label
        return want_r

    r = replay_and_check(np.stack([MR.pack_rows(range(0, 300), 1024), MR.pack_rows(range(100, 320), 1024)]),
                         [0.5, 0.5, 0.5], "first")
    assert len(mem) == 320 and (r >= 0).all() and (r[1] >= 100).all()
    src.copy_(rows[320:384])                          # the next 64 rows, another query, other lam, another mask
    q.copy_(rows[330:333])
    r = replay_and_check(np.stack([MR.pack_rows(range(300, 384), 1024), MR.pack_rows([7], 1024)]), [0.0, 1.0, 0.8],
                         "rewritten")
    assert len(mem) == 384 and (r[0] >= 300).all() and r[1].tolist() == [7] + [-1] * 5
    assert 330 in r[0].tolist() and 332 in r[2].tolist()          # the rows appended by this very replay
    mem.close()
