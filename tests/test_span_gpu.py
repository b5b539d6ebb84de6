"""GPU: the span top-k (vm_topk_cosine_span, csrc/topk_span.hip) and EmbeddingMemory.recall_links against
tests/span_ref.py.

Bar: rows, fp64 score bits and padding identical to statement (A) of the oracle, for the fast and the ``exact=True``
entry.  The scan test runs the shapes at which the shared tile scan can go wrong (tests/tile_scan_data.py) under
every span set of tests/span_ref.py and demands flag 0 of every query: the redo would hide a broken scan.  That the data
allows it is asserted from the oracle's scores before any search, and proven without a GPU in tests/test_span_cpu.py; so
is the same condition of the link test.
"""
import numpy as np
import pytest
import torch

from tests import mask_ref as MR
from tests import span_ref as SR
from tests.support import (bits, check_entries, clustered, grouped_memory, plain_memory, planted_duplicates, queries_near,
                           scan_memory, tagged_memory)
from tests.tile_scan_data import dataset

pytestmark = pytest.mark.gpu

MIN, MAX = SR.INT64_MIN, SR.INT64_MAX


def _bits64(a):
    return (a.cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.int64)


def want_of(mem, q, k, dtype, spans, **kw):
    """Statement (A) for the memory as it is."""
    base, host_rows = mem.rows_host()
    return SR.span_topk(bits(q), host_rows, spans, k, dtype=dtype, base=base, **kw)


def check(mem, q, k, dtype, spans, certified=False, label="", stride=(1, 0), **kw):
    """Fast and exact entry against (A).  certified=True: the fast path answered every query (flag 0)."""
    want_r, want_s = want_of(mem, q, k, dtype, spans, **kw)
    want_r = np.where(want_r >= 0, want_r * stride[0] + stride[1], -1)

    def call(exact):
        s, r = mem.topk_span(q, k, spans, exact=exact, stride=stride, **kw)
        return r, s
    return check_entries(call, lambda: mem.last_span_flags[:q.shape[0]], (want_r, want_s), certified or None, label)


# ---- 1. the scan ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(MR.SHAPES))
@pytest.mark.parametrize("D,dtype", [(128, "f16"), (128, "bf16"), (384, "f16"), (384, "bf16")])
def test_scan(D, dtype, shape):
    SR.scan_precondition(D, dtype, shape)            # from oracle scores, before any search
    mem, q_all, base, live, total, cap = scan_memory(D, dtype, shape)
    n = live.shape[1]
    for Q in MR.QS:
        q = q_all[:Q].contiguous()
        for name, spans in SR.span_sets(Q, shape).items():
            got_r, got_s, _ = check(mem, q, MR.K, dtype, spans, certified=True, label=f"{shape} {name} Q={Q}")
            sel = SR.selection(spans, Q, base, n)
            wr, ws = MR.masked_topk_from_scores(live[:Q], sel, MR.K, base=base)      # and (B), from the shared matrix
            assert np.array_equal(got_r, wr) and np.array_equal(got_s.view(np.int64), ws.view(np.int64)), name
            if name == "all":
                s0, r0 = mem.topk(q, MR.K)
                assert np.array_equal(r0.cpu().numpy(), got_r) and np.array_equal(_bits64(s0), got_s.view(np.int64))
            if name in ("empty", "first_dead"):
                assert (got_r == -1).all() and (got_s == 0.0).all()
            if name == "one_empty":
                assert got_r[Q // 2, 0] == -1 and (np.delete(got_r[:, 0], Q // 2) >= 0).all()
            if name == "last_live":
                assert (got_r == total - 1).all()
            if name == "below_oldest":
                assert ((got_r >= base) & (got_r <= base + 2)).all()
            if name == "seam":
                assert ((got_r >= 37) & (got_r <= 43)).all()
    mem.close()


# ---- 2. identities, bit for bit -----------------------------------------------------------------------------------------
def test_open_span_equals_topk_and_spans_equal_scopes_and_masks():
    rows, _ = clustered([5] * 800, 768, "f16", seed=3)
    mem = tagged_memory(rows, np.arange(4000), "f16")                # tag = row id
    q = queries_near(rows, 16, 9, "f16")
    ranges = [(500, 999), (33, 33), (3990, 5000), (-10, 17), (10, 5), SR.OPEN]
    per_query = [(100 * i, 100 * i + 37 * (i + 1)) for i in range(16)]
    for k in (1, 10, 50):
        s0, r0 = mem.topk(q, k)
        for span in (SR.OPEN, (None, None), (0, 3999)):
            s1, r1 = mem.topk_span(q, k, span)
            assert torch.equal(r0, r1) and np.array_equal(_bits64(s0), _bits64(s1)), (k, span)
        for span in ranges + [per_query]:
            s0, r0 = mem.topk_scoped(q, k, span)
            sel = SR.selection(span, 16, 0, 4000)
            distinct = range(16) if span is per_query else range(1)      # mask q for query q, or one mask for all
            masks = torch.stack([mem.mask_of_rows(np.nonzero(sel[i])[0].tolist()) for i in distinct])
            s2, r2 = mem.topk_masked(q, k, masks)
            for exact in (False, True):
                s1, r1 = mem.topk_span(q, k, span, exact=exact)
                assert torch.equal(r0, r1) and torch.equal(r2, r1), (k, span, exact)
                assert np.array_equal(_bits64(s0), _bits64(s1)) and np.array_equal(_bits64(s2), _bits64(s1)), (k, span, exact)
    check(mem, q, 10, "f16", per_query, stride=(3, 1), label="stride")
    s1, r1 = mem.topk_span(q, 10, per_query, stride=(3, 1))
    s0, r0 = mem.topk_span(q, 10, per_query)
    assert torch.equal(r1, torch.where(r0 >= 0, r0 * 3 + 1, r0)) and torch.equal(s0, s1)
    mem.close()


# ---- 3. the redo --------------------------------------------------------------------------------------------------------
def test_more_duplicates_than_slack_inside_the_span_is_flagged_and_redone():
    from vidmem import _lib
    rows, planted, dup = planted_duplicates()
    mem = plain_memory(rows, "f16")
    before = mem.span_uncertified_count
    got_r, _, flags = check(mem, planted[None].contiguous(), 10, "f16", (1000, 1999), label="ties inside")
    assert got_r[0].tolist() == dup[:10]               # lowest row ids first
    assert flags[0] == _lib.VM_FLAG_GAP and mem.span_uncertified_count == before + 1


def test_the_same_duplicates_outside_the_span_leave_flag_zero():
    rows, planted, dup = planted_duplicates()
    mem = plain_memory(rows, "f16")
    q = planted[None].contiguous()
    assert min(dup) >= 1010 and max(dup) < 2000
    exact = np.sort(MR.cref.cosine_matrix(bits(q), mem.rows_host()[1])[0][2000:3000])[::-1]
    assert exact[9] - exact[18] > 4 * MR.cert_eps(768), "precondition: rank k and rank M + 1 too close in the oracle"
    before = mem.span_uncertified_count
    got_r, _, _ = check(mem, q, 10, "f16", (2000, None), certified=True, label="ties outside")
    assert (got_r[0] >= 2000).all() and mem.span_uncertified_count == before


def test_more_rows_at_the_cut_than_the_select_buffer_is_an_overflow():
    """9,000 exact copies inside the span share one key, so all of them lie at the query's cut: more than the 8,192 the
    select buffer holds."""
    from vidmem import _lib
    rows = torch.randn(10000, 128, device="cuda", generator=torch.Generator("cuda").manual_seed(4)).to(torch.float16)
    rows[500:9500] = rows[3]
    mem = plain_memory(rows, "f16")
    got_r, _, flags = check(mem, rows[3:4].contiguous(), 10, "f16", (100, 9899), label="overflow")
    assert flags[0] == _lib.VM_FLAG_OVERFLOW and got_r[0].tolist() == list(range(500, 510))


def test_a_bf16_row_outside_the_norm_domain_flags_every_query_and_the_answer_is_exact():
    """One stored row of norm 2^50 sets the memory's sticky domain word (vm_memory_create: the bound holds for norms in
    [2^-40, 2^40]): the certificate is not used, every query is answered by the in-call redo."""
    rows, _ = clustered([5] * 60, 128, "bf16", seed=17)
    rows = rows.clone()
    rows[150] = (rows[150].float() * 2.0 ** 50).to(torch.bfloat16)       # a power of two: exact in bf16
    mem = plain_memory(rows, "bf16")
    q = queries_near(rows[:100].contiguous(), 5, 3, "bf16")
    spans = [(0, 99), (140, 160), (150, 150), (200, 299), (9, 3)]       # with the row, without it, empty
    got_r, _, flags = check(mem, q, 5, "bf16", spans, label="outside the domain")
    assert (flags != 0).all() and got_r[2].tolist() == [150, -1, -1, -1, -1]
    assert (got_r[4] == -1).all()


# ---- 4. the exact entry on a wrapped ring -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_exact_entry_on_a_wrapped_ring(dtype):
    """tests/test_pred_redo_gpu.py's shape: a ring of capacity 200 (not a multiple of 16) after 333 rows - rows 133 .. 332
    live, row 200 in slot 0; Q = 17 (two query tiles, the second ragged), k = 5."""
    from vidmem.memory import EmbeddingMemory
    CAP, TOTAL, D, Q, K = 200, 333, 128, 17, 5
    td = torch.float16 if dtype == "f16" else torch.bfloat16
    g = torch.Generator("cuda").manual_seed(41)
    rows = torch.randn(TOTAL, D, device="cuda", generator=g).to(td)
    mem = EmbeddingMemory(CAP, D, dtype, ring=True)
    for c0 in range(0, TOTAL, 111):          # three appends; the last one wraps
        mem.append(rows[c0:c0 + 111])
    base, host_rows = mem.rows_host()
    assert base == TOTAL - CAP and host_rows.shape[0] == CAP
    pick = torch.arange(Q, device="cuda") * 11 + base + 3
    q = (rows[pick].float() + 0.05 * torch.randn(Q, D, device="cuda", generator=g)).to(td)
    spans = [(183 + i, 204 + 3 * i) for i in range(Q)]      # row 199 sits in the last slot, row 200 in slot 0
    spans[4] = (100, 215)                    # from below the oldest live row (133)
    spans[9] = (250, 249)                    # empty
    got_r, _, _ = check(mem, q, K, dtype, spans, label="ring")
    assert (got_r[9] == -1).all() and (np.delete(got_r, 9, axis=0) >= 0).all() and (got_r[4][got_r[4] >= 0] >= 133).all()
    dev = torch.tensor(spans, dtype=torch.int64, device="cuda")           # a device tensor: not read on the host
    s1, r1 = mem.topk_span(q, K, dev, exact=True)
    assert np.array_equal(r1.cpu().numpy(), got_r)
    mem.close()


# ---- 5. arguments and memory kinds --------------------------------------------------------------------------------------
def test_arguments():
    from vidmem import _lib
    rows, _ = clustered([5] * 200, 768, "bf16", seed=12)
    mem = plain_memory(rows, "bf16")
    q = queries_near(rows, 16, 5, "bf16")
    spans = [(50 * i, 50 * i + 20 * (i + 1)) for i in range(16)]
    for score_mode, cut in ((0, 0.3), (1, 0.65), (0, None), (1, None)):
        got_r, got_s, _ = check(mem, q, 64, "bf16", spans, score_mode=score_mode, min_score=cut, label=f"mode {score_mode}")
        if cut is not None:
            assert (got_s == 0.0).any()                             # the filter cut the lists short
    got_r, _, _ = check(mem, q, 64, "bf16", spans, label="k=64")
    assert (got_r[0] >= 0).sum() == 21 and (got_r[0, 21:] == -1).all()       # k above the rows in the span
    ws = mem.prepare_topk_span(2, 3).ws
    out_s = torch.empty((2, 64), dtype=torch.float64, device="cuda")
    out_r = torch.empty((2, 64), dtype=torch.int64, device="cuda")
    sp = torch.tensor([[0, 0], [99, 99]], dtype=torch.int64, device="cuda")      # row 0 = lo, row 1 = hi

    def call(lo, hi, k, ws_bytes, exact=False):
        head = (mem.handle, q.data_ptr(), 2, k, lo, hi, 0, 0.0, 0, 1, 0, out_s.data_ptr(), out_r.data_ptr())
        tail = (ws.data_ptr(), ws_bytes, _lib.current_stream_ptr())
        if exact:
            return mem.L.vm_topk_cosine_span_exact(*head, *tail)
        return mem.L.vm_topk_cosine_span(*head, None, None, *tail)

    lo, hi = sp[0].data_ptr(), sp[1].data_ptr()
    need = int(mem.L.vm_topk_span_workspace_bytes(mem.handle, 2, 3))
    assert need == int(mem.L.vm_topk_scoped_workspace_bytes(mem.handle, 2, 3)) and ws.numel() >= need
    out_r.fill_(-7)
    for exact in (False, True):                                     # the C entry points refuse, before any launch
        assert call(None, hi, 3, ws.numel(), exact) == _lib.VM_ERR_INVALID
        assert call(lo, None, 3, ws.numel(), exact) == _lib.VM_ERR_INVALID
        assert call(lo, hi, 0, ws.numel(), exact) == _lib.VM_ERR_INVALID
        assert call(lo, hi, 65, ws.numel(), exact) == _lib.VM_ERR_INVALID
        assert call(lo, hi, 3, need - 1, exact) == _lib.VM_ERR_NOMEM
    torch.cuda.synchronize()
    assert (out_r == -7).all()                                      # nothing ran
    assert call(lo, hi, 3, ws.numel()) == _lib.VM_OK
    torch.cuda.synchronize()
    want_r, _ = want_of(mem, q[:2], 3, "bf16", (0, 99))
    assert np.array_equal(out_r.flatten()[:6].view(2, 3).cpu().numpy(), want_r)
    mem.close()


def test_memory_kinds_and_a_span_after_an_erase():
    rows, _ = clustered([5] * 60, 128, "f16", seed=23)
    q = queries_near(rows, 17, 4, "f16")
    spans = [(10 * i, 10 * i + 45) for i in range(17)]
    kinds = {
        "plain": plain_memory(rows, "f16"),
        "grouped": grouped_memory(rows, [5] * 60, "f16"),
        "tagged": tagged_memory(rows, np.arange(300) // 7, "f16"),
        "ring": plain_memory(rows, "f16", capacity=208, ring=True, step=77),      # rows 92 .. 299 live
    }
    for name, mem in kinds.items():
        check(mem, q, 7, "f16", spans, label=name)
        check(mem, q, 7, "f16", SR.OPEN, label=name + " open")
    mem = kinds["grouped"]
    erased = mem.erase(rows=list(range(40, 140)))                   # 200 rows are left, renumbered 0 .. 199
    assert erased.count == 100 and mem.sync() == 200
    got_r, _, _ = check(mem, q, 7, "f16", [(150, 260)] * 17, label="after erase")
    assert ((got_r >= 150) & (got_r <= 199)).all()                  # new ids: 200 .. 260 name no row any more
    check(mem, q, 7, "f16", spans, label="after erase, per query")
    for m in kinds.values():
        m.close()


# ---- 6. capture ---------------------------------------------------------------------------------------------------------
def test_graph_capture_append_and_span_search_replayed_with_new_spans():
    from vidmem.memory import EmbeddingMemory, SpanTopkScratch
    rows, _ = clustered([4] * 256, 768, "f16", seed=61)
    mem = EmbeddingMemory(2048, 768, "f16")
    mem.append(rows[:256])
    Q, k, B = 4, 10, 128
    mem.prepare_topk_span(Q, k)                       # the memory's counter exists before the capture
    scratch = SpanTopkScratch.for_(mem, Q, k)         # and the capture runs on a scratch the caller owns
    src = rows[256:256 + B].clone()
    q = queries_near(rows, Q, 6, "f16")
    span = torch.zeros((Q, 2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):       # one linear graph
            mem.append(src)
            out_s, out_r = mem.topk_span(q, k, span, scratch=scratch)
    torch.cuda.current_stream().wait_stream(s)
    mem.sync()                     # the capture advanced only the host mirror: back to the device count
    assert len(mem) == 256 and mem._last[SpanTopkScratch] is scratch
    for rep in range(3):
        n_now = 256 + (rep + 1) * B
        src.copy_(rows[256 + rep * B:n_now])
        q.copy_(queries_near(rows[:n_now].contiguous(), Q, 10 + rep, "f16"))
        windows = [(n_now - B, MAX), (MIN, 100 + rep), (n_now - 5, n_now + 50), (7, 3)]
        span.copy_(torch.tensor(windows, dtype=torch.int64))            # rewritten in place
        graph.replay()
        torch.cuda.synchronize()
        assert mem.sync() == n_now
        want_r, want_s = want_of(mem, q, k, "f16", windows)
        assert np.array_equal(out_r.cpu().numpy(), want_r), rep
        assert np.array_equal(_bits64(out_s), want_s.view(np.int64)), rep
        assert (out_r[0] >= n_now - B).all() and (out_r[1] <= 100 + rep).all() and (out_r[3] == -1).all()
        assert sorted(out_r[2][:5].tolist()) == list(range(n_now - 5, n_now)) and (out_r[2][5:] == -1).all()   # appended since
    mem.close()


# ---- 7. recall links ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(MR.SHAPES))
@pytest.mark.parametrize("D,dtype", [(128, "f16"), (384, "bf16")])
def test_recall_links(D, dtype, shape):
    SR.link_precondition(D, dtype, shape)            # from oracle scores, before any search
    rows, _, base, _ = dataset(D, dtype, shape)
    total, cap = MR.SHAPES[shape]
    mem = plain_memory(rows, dtype, capacity=cap, ring=cap is not None, step=19)
    live = mem.rows_host()[1]
    n = live.shape[0]
    before = mem.span_uncertified_count
    for k in SR.LINK_KS:
        for gap in SR.LINK_GAPS:
            for back in SR.LINK_BACKS:
                want_r, want_s = SR.links_ref(live, base, k, min_gap=gap, max_back=back, dtype=dtype)
                for block in (16, 256):              # several pages with a ragged last one and the seam inside; one page
                    s, r = mem.recall_links(k=k, min_gap=gap, max_back=back, block=block)
                    label = (shape, k, gap, back, block)
                    assert tuple(r.shape) == (n, k)
                    assert np.array_equal(r.cpu().numpy(), want_r), label
                    assert np.array_equal(_bits64(s), want_s.view(np.int64)), label
                assert (want_r[:gap] == -1).all() and (want_r[gap:, 0] >= 0).all()       # an empty past: all-padded
    assert mem.span_uncertified_count == before      # the precondition: nothing was left to the redo
    # a window of rows, the exact entry, a score filter
    first, count = base + 5, n - 9
    want_r, want_s = SR.links_ref(live, base, 3, first=first, count=count, min_gap=2, dtype=dtype, score_mode=1, min_score=0.7)
    for exact in (False, True):
        s, r = mem.recall_links(first, count, k=3, min_gap=2, score_mode=1, min_score=0.7, block=16, exact=exact)
        assert np.array_equal(r.cpu().numpy(), want_r) and np.array_equal(_bits64(s), want_s.view(np.int64)), exact
    mem.close()


@pytest.mark.parametrize("shape", ["n47", "ring40"])
def test_recall_links_exclude_group(shape):
    """A grouped memory whose groups are the dataset's clusters: with exclude_group a row never links into its own."""
    D, dtype = 128, "f16"
    rows, _, base, _ = dataset(D, dtype, shape)
    total, cap = MR.SHAPES[shape]
    sizes, left = [], total
    while left:
        sizes.append(min(MR.CLUSTERS[len(sizes) % len(MR.CLUSTERS)], left))
        left -= sizes[-1]
    mem = grouped_memory(rows, sizes, dtype, capacity=cap, ring=cap is not None)
    live = mem.rows_host()[1]
    group_of = mem.group_keys_host()
    assert mem.rows_host()[0] == base and len(set(group_of.tolist())) > 5
    for gap, back in ((1, None), (4, 20)):
        want_r, want_s = SR.links_ref(live, base, 3, min_gap=gap, max_back=back, group_of=group_of, dtype=dtype)
        plain_r, _ = SR.links_ref(live, base, 3, min_gap=gap, max_back=back, dtype=dtype)
        if gap == 1:
            assert not np.array_equal(want_r, plain_r)                 # without it a row's best match is in its own cluster
        for block in (16, 256):
            s, r = mem.recall_links(k=3, min_gap=gap, max_back=back, exclude_group=True, block=block)
            assert np.array_equal(r.cpu().numpy(), want_r), (shape, gap, back, block)
            assert np.array_equal(_bits64(s), want_s.view(np.int64)), (shape, gap, back, block)
        got = r.cpu().numpy()
        for i in range(got.shape[0]):
            hit = got[i][got[i] >= 0]
            assert (group_of[hit - base] != group_of[i]).all()
    with pytest.raises(ValueError, match="grouped"):
        plain_memory(rows[:16], dtype).recall_links(exclude_group=True)
    mem.close()
