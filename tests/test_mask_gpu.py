"""GPU: row masks and the masked top-k (vm_topk_cosine_masked, csrc/topk_mask.hip) against tests/mask_ref.py.

Bar: rows, fp64 score bits and padding identical to statement (A) of the oracle, for the fast and the ``exact=True``
entry.  The scan test runs the shapes at which the shared tile scan can go wrong (tests/tile_scan_data.py) under
every mask set of tests/mask_ref.py and demands flag 0 of every query: the redo would hide a broken scan.  That the data
allows it is asserted from the oracle's scores before any search, and proven without a GPU in tests/test_mask_cpu.py.
"""
import numpy as np
import pytest
import torch

from tests import mask_ref as MR
from tests import scope_ref as S
from tests.support import (ALL, bits, check_entries, clustered, contiguous_tags, dev_mask, plain_memory, planted_duplicates,
                           queries_near, scan_memory, scope_of, tagged_memory)

pytestmark = pytest.mark.gpu


def want_of(mem, q, k, dtype, masks, index, **kw):
    """Statement (A) for the memory as it is: masks / index as the call takes them (host arrays)."""
    base, host_rows = mem.rows_host()
    sel = MR.selection(masks, index, q.shape[0], base, host_rows.shape[0], mem.capacity)
    return MR.masked_topk(bits(q), host_rows, sel, k, dtype=dtype, base=base, **kw)


def check(mem, q, k, dtype, masks, index=None, certified=False, label="", **kw):
    """Fast and exact entry against (A).  certified=True: the fast path answered every query (flag 0)."""
    m = dev_mask(masks)

    def call(exact):
        s, r = mem.topk_masked(q, k, m, mask_index=index, exact=exact, **kw)
        return r, s
    return check_entries(call, lambda: mem.last_mask_flags[:q.shape[0]], want_of(mem, q, k, dtype, masks, index, **kw),
                         certified or None, label)


# ---- 1. the scan ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(MR.SHAPES))
@pytest.mark.parametrize("D,dtype", [(128, "f16"), (128, "bf16"), (384, "f16"), (384, "bf16")])
def test_scan(D, dtype, shape):
    MR.scan_precondition(D, dtype, shape)            # from oracle scores, before any search
    mem, q_all, base, live, total, cap = scan_memory(D, dtype, shape)
    assert mem.mask_words == mem.L.vm_memory_mask_words(mem.handle) == 2
    n = live.shape[1]
    for Q in MR.QS:
        q = q_all[:Q].contiguous()
        for name, (masks, index) in MR.mask_sets(Q, shape).items():
            got_r, got_s, _ = check(mem, q, MR.K, dtype, masks, index, certified=True, label=f"{shape} {name} Q={Q}")
            sel = MR.selection(masks, index, Q, base, n, mem.capacity)
            wr, ws = MR.masked_topk_from_scores(live[:Q], sel, MR.K, base=base)      # and (B), from the shared matrix
            assert np.array_equal(got_r, wr) and np.array_equal(got_s.view(np.int64), ws.view(np.int64)), name
            if name == "full":
                s0, r0 = mem.topk(q, MR.K)
                assert np.array_equal(r0.cpu().numpy(), got_r)
                assert np.array_equal(s0.cpu().numpy().view(np.int64), got_s.view(np.int64))
            if name in ("empty", "first_dead"):
                assert (got_r == -1).all() and (got_s == 0.0).all()
            if name == "one_empty":
                assert got_r[Q // 2, 0] == -1 and (np.delete(got_r[:, 0], Q // 2) >= 0).all()
            if name == "last_live":
                assert (got_r == next(r for r in range(base, base + n) if r % mem.capacity == n - 1)).all()   # slot n - 1
            if name == "newest":
                assert (got_r == total - 1).all()
            if name == "oldest":
                assert (got_r == base).all()
    mem.close()


# ---- 2. equivalences ----------------------------------------------------------------------------------------------------
def test_mask_of_scope_equals_topk_scoped_and_full_mask_equals_topk():
    rows, _ = clustered([5] * 800, 768, "f16", seed=3)
    tags = contiguous_tags(4000, 8)
    mem = tagged_memory(rows, tags, "f16")
    q = queries_near(rows, 16, 9, "f16")
    for k in (1, 10, 50):
        for sc in (scope_of(2), scope_of(5, 33 * 100, 33 * 300), (10, 5), ALL):
            m = mem.mask_of_scope(sc)
            s0, r0 = mem.topk_scoped(q, k, sc)
            for exact in (False, True):
                s1, r1 = mem.topk_masked(q, k, m, exact=exact)
                assert torch.equal(r0, r1), (k, sc, exact)
                assert np.array_equal(s0.cpu().numpy().view(np.int64), s1.cpu().numpy().view(np.int64))
        s0, r0 = mem.topk(q, k)
        s1, r1 = mem.topk_masked(q, k, ~mem.new_mask())
        assert torch.equal(r0, r1) and np.array_equal(s0.cpu().numpy().view(np.int64), s1.cpu().numpy().view(np.int64))
    # two disjoint ranges in one mask: no (lo, hi) pair can say it; against the union computed by (A)
    two = [scope_of(1), scope_of(6, 33 * 50, 33 * 200)]
    m = mem.mask_of_scope(two)
    union = S.scope_mask(tags, *two[0]) | S.scope_mask(tags, *two[1])
    assert mem.rows_of_mask(m) == union.nonzero()[0].tolist() and union.sum() == 500 + 151
    want_r, want_s = MR.masked_topk(bits(q), mem.rows_host()[1], np.tile(union, (16, 1)), 10)
    s1, r1 = mem.topk_masked(q, 10, m)
    assert np.array_equal(r1.cpu().numpy(), want_r)
    assert np.array_equal(s1.cpu().numpy().view(np.int64), want_s.view(np.int64))


# ---- 3. the redo --------------------------------------------------------------------------------------------------------
def test_more_duplicates_than_slack_inside_the_mask_is_flagged_and_redone():
    from vidmem import _lib
    rows, planted, dup = planted_duplicates()
    mem = plain_memory(rows, "f16")
    inside = MR.pack_rows(range(1000, 2000), mem.capacity)[None]
    before = mem.masked_uncertified_count
    got_r, _, flags = check(mem, planted[None].contiguous(), 10, "f16", inside, label="ties inside")
    assert got_r[0].tolist() == dup[:10]               # lowest row ids first
    assert flags[0] == _lib.VM_FLAG_GAP and mem.masked_uncertified_count == before + 1


def test_the_same_duplicates_outside_the_mask_leave_flag_zero():
    rows, planted, dup = planted_duplicates()
    mem = plain_memory(rows, "f16")
    keep = [r for r in range(3000) if r not in set(dup) and r != 5]
    outside = MR.pack_rows(keep, mem.capacity)[None]
    q = planted[None].contiguous()
    exact = np.sort(MR.cref.cosine_matrix(bits(q), mem.rows_host()[1])[0][keep])[::-1]
    assert exact[9] - exact[18] > 4 * MR.cert_eps(768), "precondition: rank k and rank M + 1 too close in the oracle"
    before = mem.masked_uncertified_count
    got_r, _, flags = check(mem, q, 10, "f16", outside, certified=True, label="ties outside")
    assert not set(got_r[0].tolist()) & set(dup + [5]) and mem.masked_uncertified_count == before


def test_more_rows_at_the_cut_than_the_select_buffer_is_an_overflow():
    """9,000 exact copies inside the mask share one key, so all of them lie at the query's cut: more than the 8,192 the
    select buffer holds.  (tests/test_scope_topk_gpu.py has no overflow case; tied rows are the direct construction.)"""
    from vidmem import _lib
    rows = torch.randn(10000, 128, device="cuda", generator=torch.Generator("cuda").manual_seed(4)).to(torch.float16)
    rows[500:9500] = rows[3]
    mem = plain_memory(rows, "f16")
    inside = MR.pack_rows(range(100, 9900), mem.capacity)[None]
    got_r, _, flags = check(mem, rows[3:4].contiguous(), 10, "f16", inside, label="overflow")
    assert flags[0] == _lib.VM_FLAG_OVERFLOW and got_r[0].tolist() == list(range(500, 510))


# ---- 4. the builders ----------------------------------------------------------------------------------------------------
def test_builders_on_a_ring():
    rows, _ = clustered([3] * 19, 128, "f16", seed=5)
    tags = np.arange(57, dtype=np.int64) // 10                      # six sources of ten rows
    mem = tagged_memory(rows, tags, "f16", capacity=40, ring=True, step=19)      # rows 17 .. 56 live
    q = torch.cat([rows[30:31], rows[30:31], rows[50:51]]).contiguous()
    few = MR.pack_rows([28, 29, 30, 31, 50], 40)[None]
    _, r = mem.topk_masked(q, 8, dev_mask(few))                     # 5 selected rows, k = 8: -1 padding, duplicates
    assert (r[:, 5:] == -1).all() and torch.equal(r[0], r[1])
    m = mem.mask_of_rows(r)                                         # a device tensor: not read on the host
    assert mem.rows_of_mask(m) == [28, 29, 30, 31, 50]
    assert np.array_equal(m.cpu().numpy().view(np.uint32), MR.pack_rows([28, 29, 30, 31, 50], 40))
    ids = torch.tensor([3, 16, 17, 56, 57, 1000, -1, 56, -5], dtype=torch.int64, device="cuda")
    assert mem.rows_of_mask(mem.mask_of_rows(ids)) == [17, 56]      # 3, 16: overwritten; 57, 1000: never appended
    assert mem.rows_of_mask(mem.mask_of_rows([40, 39])) == [39, 40]  # a host sequence; slots 0 and 39
    out = mem.new_mask()
    assert mem.mask_of_rows([20], out=out[0]).data_ptr() == out.data_ptr() and mem.rows_of_mask(out) == [20]
    mem.mask_of_rows(ids, out=out[0], clear=False)
    assert mem.rows_of_mask(out) == [17, 20, 56]                    # ORed into what was there
    mem.mask_of_rows([21], out=out[0])
    assert mem.rows_of_mask(out) == [21]                            # cleared first
    mem.mask_of_rows([], out=out[0])
    assert mem.rows_of_mask(out) == [] and not out.any()
    # strided ids, as a sharded search writes them
    wide = torch.tensor([30 * 4 + 1, 31 * 4 + 2, 32 * 4 + 1, 5], dtype=torch.int64, device="cuda")
    mem.ctx.check(mem.L.vm_mask_from_rows(mem.handle, wide.data_ptr(), 4, 4, 1, 1, out.data_ptr(), None))
    assert mem.rows_of_mask(out) == [30, 32]
    # scopes against numpy on the tags
    live_tags = mem.tags_host()
    for sc in ((2, 3), [(1, 1), (4, 5)], (7, 9), (3, 2), ALL):
        pairs = [sc] if not isinstance(sc, list) else sc
        hit = np.zeros(40, dtype=bool)
        for lo, hi in pairs:
            hit |= S.scope_mask(live_tags, lo, hi)
        m = mem.mask_of_scope(sc)
        assert mem.rows_of_mask(m) == (17 + hit.nonzero()[0]).tolist(), sc
        assert np.array_equal(m.cpu().numpy().view(np.uint32), MR.pack_rows(17 + hit.nonzero()[0], 40)), sc   # dead = 0
    excl = ~mem.mask_of_rows([30, 31]) & mem.mask_of_scope((3, 3))
    assert mem.rows_of_mask(excl) == [32, 33, 34, 35, 36, 37, 38, 39]
    check(mem, q, 5, "f16", excl.cpu().numpy().view(np.uint32)[None], label="exclusion")
    with pytest.raises(ValueError, match="tagged"):
        plain_memory(rows[:16], "f16").mask_of_scope((0, 1))


# ---- 5. arguments -------------------------------------------------------------------------------------------------------
def test_arguments():
    from vidmem import _lib
    rows, _ = clustered([5] * 200, 768, "bf16", seed=12)
    mem = plain_memory(rows, "bf16", grouped=True)                  # any memory: here a grouped one
    q = queries_near(rows, 16, 5, "bf16")
    rng = np.random.default_rng(1)
    masks = np.stack([MR.pack_rows(np.nonzero(rng.random(1000) < p)[0], 1000) for p in (0.5, 0.1, 0.03)])
    index = [i % 3 for i in range(16)]
    for score_mode, cut in ((0, 0.3), (1, 0.65), (0, None), (1, None)):
        got_r, got_s, _ = check(mem, q, 64, "bf16", masks, index, score_mode=score_mode, min_score=cut, label=f"mode {score_mode}")
        if cut is not None:
            assert (got_s == 0.0).any()                             # the filter cut the lists short
    got_r, _, _ = check(mem, q, 64, "bf16", masks, index, label="k=64")
    few = int(MR.selected(masks[2], 0, 1000, 1000).sum())
    assert few < 64 and ((got_r[2] >= 0).sum() == few) and (got_r[2, few:] == -1).all()     # k above the selected rows
    got_r, got_s, flags = check(mem, q[:4].contiguous(), 5, "bf16", masks, [0, 3, -1, 1 << 30], label="index out of range")
    assert (got_r[1:] == -1).all() and (got_s[1:] == 0.0).all() and (flags[1:] == 0).all()      # padded, no fault
    assert (got_r[0] >= 0).all()
    with pytest.raises(ValueError, match="width"):
        mem.topk_masked(q, 3, torch.zeros(mem.mask_words + 2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="mask_index"):
        mem.topk_masked(q, 3, dev_mask(masks))                      # 3 masks, 16 queries, no index
    ws = mem.prepare_topk_masked(2, 3).ws
    out_s = torch.empty((2, 64), dtype=torch.float64, device="cuda")
    out_r = torch.empty((2, 64), dtype=torch.int64, device="cuda")
    m = dev_mask(masks)
    for n_masks, k in ((3, 3), (1, 0), (1, 65), (0, 3)):            # the C entry point refuses too
        rc = mem.L.vm_topk_cosine_masked(mem.handle, q.data_ptr(), 2, k, m.data_ptr(), n_masks, None, 0, 0.0, 0, 1, 0,
                                         out_s.data_ptr(), out_r.data_ptr(), None, None, ws.data_ptr(), ws.numel(),
                                         _lib.current_stream_ptr())
        assert rc == _lib.VM_ERR_INVALID, (n_masks, k)


# ---- 6. capture ---------------------------------------------------------------------------------------------------------
def test_graph_capture_replayed_after_a_mask_rewrite_and_an_append():
    from vidmem.memory import EmbeddingMemory, MaskedTopkScratch
    rows, _ = clustered([4] * 128, 768, "f16", seed=61)
    mem = EmbeddingMemory(1024, 768, "f16")
    mem.append(rows[:256])
    Q, k = 4, 10
    mem.prepare_topk_masked(Q, k)                     # the memory's counter exists before the capture
    scratch = MaskedTopkScratch.for_(mem, Q, k)       # and the capture runs on a scratch the caller owns
    q = queries_near(rows, Q, 6, "f16")
    mask = mem.new_mask(2)
    index = torch.tensor([0, 1, 0, 1], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):       # one linear graph
            out_s, out_r = mem.topk_masked(q, k, mask, mask_index=index, scratch=scratch)
    torch.cuda.current_stream().wait_stream(s)
    assert mem._own[MaskedTopkScratch] is not scratch and mem._last[MaskedTopkScratch] is scratch

    def replay_and_check(words, label):
        mask.copy_(dev_mask(words))                   # rewritten in place
        graph.replay()
        torch.cuda.synchronize()
        want_r, want_s = want_of(mem, q, k, "f16", words, [0, 1, 0, 1])
        assert np.array_equal(out_r.cpu().numpy(), want_r), label
        assert np.array_equal(out_s.cpu().numpy().view(np.int64), want_s.view(np.int64)), label
        return want_r

    r = replay_and_check(np.stack([MR.pack_rows(range(0, 128), 1024), MR.pack_rows(range(100, 256), 1024)]), "first")
    assert (r[0] < 128).all() and (r[1] >= 100).all()
    r = replay_and_check(np.stack([MR.pack_rows(range(200, 400), 1024), MR.pack_rows([7], 1024)]), "rewritten")
    assert ((r[0] >= 200) & (r[0] < 256)).all() and r[1].tolist() == [7] + [-1] * 9      # rows 256 .. 399 are not live yet
    mem.append(rows[256:512])
    q.copy_(rows[[300, 301, 310, 320]])
    r = replay_and_check(np.stack([MR.pack_rows(range(200, 400), 1024), MR.pack_rows(range(0, 512, 2), 1024)]), "appended")
    assert r[0, 0] == 300 and r[1, 0] in (300, 302) and r[2, 0] == 310 and r[3, 0] == 320   # the rows appended since
    assert (r[1] % 2 == 0).all()
