"""CPU: the two statements of the span top-k oracle (tests/span_ref.py) against each other and the link loop against
both, the host-side rules of the span search and of recall_links (scratch owner rule, refusals, adapter exclusions, header
text, exported symbols), and the data preconditions of the GPU tests (tests/test_span_gpu.py, tests/test_span_e2e_gpu.py),
proven here from the oracle alone."""
import os
import re

import numpy as np
import pytest
import torch

from tests import mask_ref as MR
from tests import span_ref as SR
from tests.host_memory import host_memory, owner_rule_holds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN, MAX = SR.INT64_MIN, SR.INT64_MAX


def _case(seed, n=3000, D=768, Q=12, base=7):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, D)).astype(np.float16)
    for i in range(0, 200, 7):                       # planted exact duplicates, inside spans and outside
        rows[rng.integers(0, n)] = rows[i]
    q = rows[rng.integers(0, n, Q)].astype(np.float32) + 0.1 * rng.standard_normal((Q, D)).astype(np.float32)
    q = q.astype(np.float16)
    q[3] = rows[0]
    q[4] = 0
    lo = base + rng.integers(0, n, Q)
    spans = [(int(a), int(a + rng.integers(0, n))) for a in lo]          # some reach past the newest row
    spans[0] = (base + 50, base + 49)                # empty
    spans[1] = SR.OPEN                               # every row
    spans[2] = (base + 17, base + 17)                # one row
    spans[3] = (MIN, base + 100)                     # open below
    spans[5] = (base - 40, base + 3)                 # from below the oldest row
    spans[6] = (base + n, MAX)                       # ids at and past the row count only
    return q.view(np.uint16), rows.view(np.uint16), spans, base


@pytest.mark.parametrize("score_mode,min_score", [(0, None), (0, 0.3), (1, 0.65)])
@pytest.mark.parametrize("seed", [0, 1])
def test_two_statements_agree(seed, score_mode, min_score):
    q, rows, spans, base = _case(seed)
    sel = SR.selection(spans, q.shape[0], base, rows.shape[0])
    assert not sel[0].any() and sel[1].all() and sel[2].sum() == 1 and sel[3].sum() == 101 and sel[5].sum() == 4
    assert not sel[6].any()
    for k in (1, 10, 64):
        ra, sa = SR.span_topk(q, rows, spans, k, "f16", score_mode, min_score, base=base)
        rb, sb = SR.span_topk_matrix(q, rows, spans, k, "f16", score_mode, min_score, base=base)
        assert np.array_equal(ra, rb)
        assert np.array_equal(sa.view(np.int64), sb.view(np.int64))
        assert (ra[0] == -1).all() and (sa[0] == 0.0).all() and (ra[2, 1:] == -1).all() and (ra[6] == -1).all()
        rm, sm = MR.masked_topk(q, rows, sel, k, "f16", score_mode, min_score, base=base)     # the masked oracle's (A)
        assert np.array_equal(ra, rm) and np.array_equal(sa.view(np.int64), sm.view(np.int64))
    r, _ = SR.span_topk(q, rows, spans, 64, "f16", score_mode, min_score, base=base)
    for qi in range(q.shape[0]):                     # only rows in the span are ever returned
        got = r[qi][r[qi] >= 0]
        assert sel[qi][got - base].all()


def test_the_open_span_equals_the_row_ranking():
    from oracle import cref
    q, rows, _, _ = _case(5, n=500, D=128, Q=8)
    r0, s0 = cref.cosine_topk(q, rows, 20)
    for span in (SR.OPEN, (None, None), (0, 499), (-3, 10 ** 12)):
        r1, s1 = SR.span_topk(q, rows, span, 20)
        assert np.array_equal(r0, r1) and np.array_equal(s0.view(np.int64), s1.view(np.int64))


def test_ties_by_row_id_and_zero_query():
    rows = np.zeros((6, 128), dtype=np.float16)
    rows[:, 0] = 1.0
    rows[2, 0], rows[2, 1] = 0.5, 1.0                # rows 0, 1, 3, 4, 5 are one vector, row 2 another
    q = np.zeros((2, 128), dtype=np.float16)
    q[0, 0] = 1.0                                    # query 1 is the zero vector: every score is 0.0
    for fn in (SR.span_topk, SR.span_topk_matrix):
        r, s = fn(q.view(np.uint16), rows.view(np.uint16), (11, 14), 3, base=10)     # rows 11 .. 14 of 10 .. 15
        assert r.tolist() == [[11, 13, 14], [11, 12, 13]] and s[1].tolist() == [0.0] * 3 and s[0, 0] == 1.0


def test_links_loop_against_both_statements():
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((90, 128)).astype(np.float16).view(np.uint16)
    group_of = np.repeat(np.arange(30), 3) + 100     # groups of three rows
    base = 12
    for kw in (dict(min_gap=1), dict(min_gap=4, max_back=20), dict(min_gap=1, group_of=group_of),
               dict(min_gap=2, max_back=7, group_of=group_of)):
        spans = SR.link_spans(base, 90, base, **kw)
        if "group_of" in kw:                         # never a row of the query's own group, nor anything after it
            assert all(hi < base + (i // 3) * 3 for i, (lo, hi) in enumerate(spans))
        lr, ls = SR.links_ref(rows, base, 5, **kw)
        for fn in (SR.span_topk, SR.span_topk_matrix):
            r, s = fn(rows, rows, spans, 5, base=base)
            assert np.array_equal(lr, r) and np.array_equal(ls.view(np.int64), s.view(np.int64))
        assert (lr[0] == -1).all()                   # the oldest row has no past
        live = lr >= 0
        assert (lr[live] <= (np.arange(base, base + 90)[:, None] - kw["min_gap"]).repeat(5, 1)[live]).all()
    lr, _ = SR.links_ref(rows, base, 2, first=base + 40, count=10, min_gap=3)
    full, _ = SR.links_ref(rows, base, 2, min_gap=3)
    assert np.array_equal(lr, full[40:50])


# ---- the scratch owner rule for the new kind (tests/host_memory.py's stand-in sizing library) -------------------
def test_span_scratch_follows_the_owner_rule():
    from vidmem import memory as M
    mem = owner_rule_holds("SpanTopkScratch", "prepare_topk_span")
    assert mem.last_span_flags is None and mem.span_uncertified_count == 0
    assert M.SpanTopkScratch.workspaces == (("ws", "vm_topk_span_workspace_bytes"),)


# ---- refusals, before the library is called (host_memory's library fails the test when reached) ----------------------
def test_python_refusals():
    mem = host_memory(capacity=100)
    q = [[0.0] * mem.dim]
    for k in (0, 65):
        with pytest.raises(ValueError, match="k"):
            mem.topk_span(q, k, (0, 5))
        with pytest.raises(ValueError, match="k"):
            mem.recall_links(k=k)
    for bad, what in ((torch.zeros((1, 2), dtype=torch.int32), "int64"), (torch.zeros((1, 3), dtype=torch.int64), "int64"),
                      (torch.zeros(2, dtype=torch.int64), "int64"), (torch.zeros((3, 2), dtype=torch.int64), "3 spans for 1"),
                      ([(0, 1), (2, 3)], "2 spans for 1"), ([(0, 1, 2)], "pair"), ([5], "pair"), ([], "0 spans for 1")):
        with pytest.raises(ValueError, match=what):
            mem.topk_span(q, 3, bad)
    with pytest.raises(ValueError, match="min_gap"):
        mem.recall_links(min_gap=0)
    with pytest.raises(ValueError, match="max_back"):
        mem.recall_links(max_back=-1)
    with pytest.raises(ValueError, match="block"):
        mem.recall_links(block=0)
    with pytest.raises(ValueError, match="grouped"):
        mem.recall_links(exclude_group=True)
    # the host forms of a span: one pair for all, open bounds, one pair per query
    assert mem._open_spans((3, None)) == (3, MAX) and mem._open_spans([None, 9]) == (MIN, 9)
    assert mem._open_spans([(None, None), (1, 2)]) == [(MIN, MAX), (1, 2)]
    sc = mem._scopes(mem._open_spans((None, 4)), 3, "span")
    assert sc.dtype == torch.int64 and sc.tolist() == [[MIN] * 3, [4] * 3]


def test_recall_links_refuses_rows_that_are_not_live():
    sized = type("Sized", (), {"vm_memory_size": lambda self, h: 57})()
    mem = host_memory(capacity=40, library=sized)
    mem.ring = True                                  # rows 17 .. 56 live
    for kw in (dict(first_row=16), dict(first_row=50, n_rows=8), dict(first_row=20, n_rows=-1)):
        with pytest.raises(ValueError, match="not all live"):
            mem.recall_links(**kw)
    s, r = mem.recall_links(first_row=30, n_rows=0, k=3)                 # no rows: nothing reaches the library
    assert tuple(s.shape) == tuple(r.shape) == (0, 3)


class _FakeMemory:
    grouped = False
    tagged = False
    dim = 768
    searchable = 10

    def __len__(self):
        return 25


class _FakeTaggedGrouped(_FakeMemory):
    grouped = True
    tagged = True


def test_adapters_refuse_span_with_scope_mask_or_distinct():
    from vidmem import _lib
    from vidmem.similarity import HipPreLLMSimilarity, HipVectorSearch, _span_rows, batch_similarities
    m = torch.zeros(2, dtype=torch.int32)
    q = [[0.0] * 768]
    with pytest.raises(ValueError, match="span and scope are mutually exclusive"):
        batch_similarities(_FakeTaggedGrouped(), q, 3, scope=(0, 10), span=(0, 5))
    with pytest.raises(ValueError, match="span and mask are mutually exclusive"):
        batch_similarities(_FakeMemory(), q, 3, mask=m, span=(0, 5))
    with pytest.raises(ValueError, match="span and distinct=True are mutually exclusive"):
        batch_similarities(_FakeTaggedGrouped(), q, 3, distinct=True, span=(0, 5))
    with pytest.raises(ValueError, match="one pair"):
        batch_similarities(_FakeMemory(), q, 3, span=[(0, 5), (1, 2)])
    with pytest.raises(ValueError, match="mutually exclusive"):
        HipPreLLMSimilarity(_FakeTaggedGrouped(), object(), scope=(0, 10), span=(0, 5))
    with pytest.raises(ValueError, match="mutually exclusive"):
        HipPreLLMSimilarity(_FakeMemory(), object(), mask=m, span=(0, 5))
    with pytest.raises(ValueError, match="mutually exclusive"):
        HipVectorSearch(_FakeTaggedGrouped(), object(), object(), score_mode=_lib.VM_SCORE_RAW, distinct=True, span=(0, 5))
    assert HipVectorSearch(_FakeMemory(), object(), object(), score_mode=_lib.VM_SCORE_RAW, span=(None, 5)).span == (None, 5)
    assert HipPreLLMSimilarity(_FakeMemory(), object(), span=(3, None)).span == (3, None)
    # the wrong-length rule's rows: 25 rows appended, 10 searchable -> 15 .. 24 live
    assert list(_span_rows(_FakeMemory(), (None, None))) == list(range(15, 25))
    assert list(_span_rows(_FakeMemory(), (0, 17))) == [15, 16, 17] and list(_span_rows(_FakeMemory(), (23, 99))) == [23, 24]
    assert list(_span_rows(_FakeMemory(), (20, 19))) == [] and list(_span_rows(_FakeMemory(), (30, None))) == []


def test_attach_memory_takes_span():
    import inspect
    from vidmem.fusion import HipHybridMixin
    assert "span" in inspect.signature(HipHybridMixin.attach_memory).parameters


# ---- the header and the library --------------------------------------------------------------------------------------
def test_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "vidmem.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("inclusive LOCAL row ids: append order, before the row_stride / row_offset mapping",
                   "Row r counts for query q iff r is live and row_lo[q] <= r <= row_hi[q]",
                   "with lo = n - capacity in a wrapped ring",
                   "ids below the oldest row, ids at or past the row count, negative ids",
                   "row_lo[q] > row_hi[q] is the EMPTY span and gives an all-padded result row",
                   "INT64_MIN .. INT64_MAX is every live row",
                   "goes stale after an erase, exactly as a mask does",
                   "with every span INT64_MIN .. INT64_MAX the result equals vm_topk_cosine + vm_topk_redo_flagged",
                   "on a tagged memory whose tags are the row ids it equals vm_topk_cosine_scoped for the same ranges",
                   "it equals vm_topk_cosine_masked with the mask of the span's rows",
                   "the best M = k + max(8, k/4) in-span rows are re-scored exactly",
                   "the test reads no memory",
                   "a replay sees spans rewritten in place and the rows appended since",
                   "an undersized workspace is VM_ERR_NOMEM before any launch"):
        assert phrase in flat, phrase
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for decl in (r"size_t vm_topk_span_workspace_bytes\(const vm_memory \*mem, int Q, int k\);",
                 r"int vm_topk_cosine_span\(vm_memory \*mem, const void \*queries, int Q, int k, const int64_t \*row_lo, "
                 r"const int64_t \*row_hi,\s+int use_min_score, double min_score, int score_mode, int64_t row_stride, "
                 r"int64_t row_offset,\s+double \*out_scores, int64_t \*out_rows, int32_t \*out_uncertified, "
                 r"int32_t \*out_query_flags,\s+void \*workspace, size_t workspace_bytes, void \*stream\);",
                 r"int vm_topk_cosine_span_exact\(vm_memory \*mem, const void \*queries, int Q, int k, const int64_t \*row_lo,"
                 r"\s+const int64_t \*row_hi, int use_min_score, double min_score, int score_mode,\s+int64_t row_stride, "
                 r"int64_t row_offset, double \*out_scores, int64_t \*out_rows,\s+void \*workspace, size_t workspace_bytes, "
                 r"void \*stream\);"):
        assert re.search(decl, code), decl


def test_library_exports_the_span_symbols_and_abi_4():
    from vidmem import _lib
    L = _lib.lib()
    assert L.vm_abi_version() == 4
    for sym in ("vm_topk_span_workspace_bytes", "vm_topk_cosine_span", "vm_topk_cosine_span_exact"):
        assert sym in _lib.SYMBOLS
        getattr(L, sym)
    assert L.vm_topk_span_workspace_bytes(None, 1, 1) == 0
    assert L.vm_topk_cosine_span(None, None, 1, 1, None, None, 0, 0.0, 0, 1, 0, None, None, None, None, None, 0,
                                 None) == _lib.VM_ERR_INVALID
    assert L.vm_topk_cosine_span_exact(None, None, 1, 1, None, None, 0, 0.0, 0, 1, 0, None, None, None, 0,
                                       None) == _lib.VM_ERR_INVALID


# ---- the GPU tests' preconditions ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(MR.SHAPES))
@pytest.mark.parametrize("D,dtype", [(128, "f16"), (128, "bf16"), (384, "f16"), (384, "bf16")])
def test_scan_test_inputs_leave_no_query_to_the_redo(D, dtype, shape):
    """For every data set, Q and span set of tests/test_span_gpu.py's scan test: the exact best and 10th in-span scores lie
    more than 4 x cert_eps(D) apart, or fewer than 10 rows are in the span - the certificate needs 2 x, so a query the fast
    entry flags there is a scan that went wrong, not data that asked for the redo.  (41 sets x 67 queries x 4 = 10,988.)"""
    total, cap = MR.SHAPES[shape]
    assert SR.scan_precondition(D, dtype, shape) == (11 if cap else 10) * sum(MR.QS)
    n, base = min(total, cap or total), (total - cap if cap else 0)
    sets = SR.span_sets(33, shape)
    count = {name: SR.selection(sp, 33, base, n).sum(axis=1) for name, sp in sets.items()}
    assert (count["all"] == n).all() and (count["empty"] == 0).all() and (count["first_dead"] == 0).all()
    assert (count["last_live"] == 1).all() and (count["first_tile"] == 16).all() and (count["across_tiles"] == min(11, n - 10)).all()
    assert (count["below_oldest"] == 3).all() and count["one_empty"][16] == 0 and count["one_empty"].sum() == 32 * n
    assert count["causal"].tolist() == [(7 * i) % n + 1 for i in range(33)]
    assert count["staggered"].tolist() == [min(13, n - (3 * i) % n) for i in range(33)]
    if cap:                                          # slot 0 holds row 40: three rows to either side of the seam
        assert sets["seam"][0] == (37, 43) and (count["seam"] == 7).all()


@pytest.mark.parametrize("shape", list(MR.SHAPES))
@pytest.mark.parametrize("D,dtype", [(128, "f16"), (128, "bf16"), (384, "f16"), (384, "bf16")])
def test_link_test_inputs_leave_no_query_to_the_redo(D, dtype, shape):
    """The same for the link test: the stored rows as queries, k in {1, 3}, min_gap in {1, 4, 16}, max_back in {None, 20}
    (137 rows x 12 parameter sets x 4 = 6,576)."""
    total, cap = MR.SHAPES[shape]
    assert SR.link_precondition(D, dtype, shape) == min(total, cap or total) * 12


def test_e2e_noise_keeps_the_aligned_row_first():
    """tests/test_span_e2e_gpu.py: every row of A' has, among the rows at least 16 before it, its aligned row of A as the
    oracle's top hit, by more than the certificate needs against rank M + 1."""
    from oracle import cref
    rows = SR.e2e_videos()
    A, B = SR.E2E_A, SR.E2E_B
    assert rows.shape == (2 * A + B, SR.E2E_D)
    lr, ls = SR.links_ref(rows, 0, 1, first=A + B, count=A, min_gap=SR.E2E_GAP)
    assert lr[:, 0].tolist() == list(range(A)) and (ls[:, 0] > 0.9).all()
    near, _ = SR.links_ref(rows, 0, 1, first=0, count=A, min_gap=1)                # what the gap keeps out: in its first
    assert near[1:, 0].tolist() == list(range(A - 1))                              # showing a frame's best match is the one before
    scores = cref.cosine_matrix(rows[A + B:], rows)
    for i, sp in enumerate(SR.link_spans(A + B, A, 0, SR.E2E_GAP)):
        a, b = SR.clamp(sp, 0, rows.shape[0])
        assert SR.gap_ok(np.sort(scores[i, a:b])[::-1], SR.E2E_D, 1)
