"""Test oracle of the span top-k and of the recall links (include/vidmem.h vm_topk_cosine_span).

Contract: row r counts for query q iff r is live and row_lo[q] <= r <= row_hi[q], inclusive LOCAL row ids; ids that are
not live are ignored and lo > hi is the empty span.  The result is the exhaustive row ranking of vm_topk_cosine - raw
reference cosines ranked by (score desc, row id asc), the score_mode mapping, the ``> min_score`` filter on the mapped
score - taken over the rows in the span only, first k; -1 / 0.0 padded.  Two independent statements and one loop:

  (A) ``span_topk``         oracle.cref.cosine_topk (the C restatement of the reference ranking) on the CONTIGUOUS SLICE of
                            live rows the span holds, its indices mapped back to row ids;
  (B) ``span_topk_matrix``  oracle.cref.cosine_matrix over all rows, restricted to the span, the raw scores ranked by
                            (score desc, row asc), then mapped and filtered (tests/mask_ref.py's ranking of a selection);
  ``links_ref``             the per-row loop of EmbeddingMemory.recall_links: query i is the stored row first + i, its span
                            [r - max_back, r - min_gap], cut before the first row of r's own group when asked.

tests/test_span_cpu.py holds (A) against (B); the GPU tests compare with (A).  Also here: the span sets of the scan test
(tests/test_span_gpu.py) and the data preconditions of the scan and link tests, which the CPU file proves without a GPU.
"""
from __future__ import annotations

import numpy as np

from oracle import cref
from tests import mask_ref as MR

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
OPEN = (INT64_MIN, INT64_MAX)
LINK_KS, LINK_GAPS, LINK_BACKS = (1, 3), (1, 4, 16), (None, 20)    # the link test's parameters


def clamp(span, base: int, n: int):
    """One (lo, hi) in row ids -> (first, last + 1) as indices among the live rows base .. base + n - 1; first >= last + 1
    when the span holds no live row.  Python ints: no bound overflows."""
    lo, hi = int(span[0]), int(span[1])
    return max(lo, base) - base, min(hi, base + n - 1) - base + 1


def pairs(spans, Q: int):
    """One (lo, hi) for all queries or Q of them -> a list of Q pairs, ``None`` bounds opened."""
    spans = list(spans)
    if len(spans) == 2 and not hasattr(spans[0], "__len__"):
        spans = [spans] * Q
    assert len(spans) == Q, (len(spans), Q)
    return [(INT64_MIN if lo is None else int(lo), INT64_MAX if hi is None else int(hi)) for lo, hi in spans]


def selection(spans, Q: int, base: int, n: int) -> np.ndarray:
    """bool [Q, n]: which of the live rows each query's span holds."""
    sel = np.zeros((Q, n), dtype=bool)
    for q, sp in enumerate(pairs(spans, Q)):
        a, b = clamp(sp, base, n)
        if a < b:
            sel[q, a:b] = True
    return sel


def span_topk(queries, rows, spans, k, dtype="f16", score_mode=0, min_score=None, base=0):
    """(A).  queries [Q,D], rows [n,D] (uint16 bit patterns) in row-id order, the live rows base .. base + n - 1 ->
    (rows [Q,k] int64, scores [Q,k] fp64)."""
    queries = np.ascontiguousarray(queries)
    rows = np.ascontiguousarray(rows)
    Q, n = queries.shape[0], rows.shape[0]
    out_r = np.full((Q, k), -1, np.int64)
    out_s = np.zeros((Q, k), np.float64)
    same = {}
    for q, sp in enumerate(pairs(spans, Q)):
        same.setdefault(clamp(sp, base, n), []).append(q)
    for (a, b), qs in same.items():         # queries of one span share one slice of the memory
        if a >= b:
            continue
        r, s = cref.cosine_topk(queries[qs], rows[a:b], k, dtype=dtype, score_mode=score_mode, min_score=min_score)
        out_r[qs] = np.where(r >= 0, base + a + r, -1)
        out_s[qs] = s
    return out_r, out_s


def span_topk_matrix(queries, rows, spans, k, dtype="f16", score_mode=0, min_score=None, base=0):
    """(B)."""
    sel = selection(spans, np.asarray(queries).shape[0], base, np.asarray(rows).shape[0])
    return MR.masked_topk_from_scores(cref.cosine_matrix(queries, rows, dtype=dtype), sel, k, score_mode, min_score, base)


def link_spans(first, count, base, min_gap=1, max_back=None, group_of=None):
    """The span of every query of recall_links: row r = first + i sees [r - max_back, r - min_gap], open below without
    ``max_back``; with ``group_of`` (the group of every live row, in row order) it ends no later than the row before the
    first live row of r's own group."""
    spans = []
    for r in range(first, first + count):
        lo = INT64_MIN if max_back is None else r - max_back
        hi = r - min_gap
        if group_of is not None:
            g = group_of[r - base]
            start = r
            while start > base and group_of[start - 1 - base] == g:
                start -= 1
            hi = min(hi, start - 1)
        spans.append((lo, hi))
    return spans


def links_ref(rows, base, k, first=None, count=None, min_gap=1, max_back=None, group_of=None, dtype="f16", score_mode=0,
              min_score=None):
    """The per-row loop of recall_links over rows [n,D] (uint16, row-id order, live rows base .. base + n - 1): one
    restricted reference ranking per stored row -> (rows [count,k], scores [count,k])."""
    rows = np.ascontiguousarray(rows)
    n = rows.shape[0]
    first = base if first is None else first
    count = base + n - first if count is None else count
    out_r = np.full((count, k), -1, np.int64)
    out_s = np.zeros((count, k), np.float64)
    for i, sp in enumerate(link_spans(first, count, base, min_gap, max_back, group_of)):
        a, b = clamp(sp, base, n)
        if a >= b:
            continue
        q = rows[first + i - base][None]
        r, s = cref.cosine_topk(q, rows[a:b], k, dtype=dtype, score_mode=score_mode, min_score=min_score)
        out_r[i] = np.where(r[0] >= 0, base + a + r[0], -1)
        out_s[i] = s[0]
    return out_r, out_s


# ---- the scan test's span sets --------------------------------------------------------------------------------------
def span_sets(Q: int, shape: str):
    """name -> Q pairs (lo, hi) of the scan test, for a memory of mask_ref.SHAPES[shape]; base = the oldest live id,
    total = the rows appended."""
    total, cap = MR.SHAPES[shape]
    capacity = cap or total
    n = min(total, capacity)
    base = total - n
    sets = {
        "all": [OPEN] * Q,
        "empty": [(5, 4)] * Q,
        "one_empty": [(5, 4) if i == Q // 2 else OPEN for i in range(Q)],
        "first_tile": [(base, base + 15)] * Q,                       # every other tile takes the skip path
        "across_tiles": [(base + 10, base + 20)] * Q,
        "last_live": [(total - 1, total - 1)] * Q,                   # the newest row
        "first_dead": [(total, total + 100)] * Q,                    # ids at and past the row count
        "below_oldest": [(base - 7, base + 2)] * Q,                  # reaches below the oldest row (negative ids at base 0)
        "causal": [(INT64_MIN, base + (7 * i) % n) for i in range(Q)],
        "staggered": [(base + (3 * i) % n, base + (3 * i) % n + 12) for i in range(Q)],
    }
    if cap:
        seam = next(r for r in range(base, total) if r % capacity == 0)      # the id in physical slot 0
        sets["seam"] = [(seam - 3, seam + 3)] * Q
    return sets


def gap_ok(best_first, D, k) -> bool:
    """mask_ref.gap_ok for any k: rank k and rank M + 1 = k + 8 + 1 are more than 4 x cert_eps apart, or there is no
    rank M + 1 (everything is re-scored exactly)."""
    m1 = k + max(8, k // 4) + 1
    if k == MR.K:
        assert m1 == MR.M1
        return MR.gap_ok(best_first, D)
    return best_first.size < m1 or bool(best_first[min(k, best_first.size) - 1] - best_first[m1 - 1] > 4 * MR.cert_eps(D))


def scan_precondition(D, dtype, shape) -> int:
    """Asserts, from the oracle's scores alone, that no query of any span set of the scan test is left to the redo; -> the
    number of (query, set) cases checked."""
    _, _, base, live = MR.host_dataset(D, dtype, shape)
    n = live.shape[1]
    cases = 0
    for Q in MR.QS:
        for name, spans in span_sets(Q, shape).items():
            sel = selection(spans, Q, base, n)
            for i in range(Q):
                assert MR.gap_ok(np.sort(live[i][sel[i]])[::-1], D), f"precondition: {shape} D={D} {dtype} {name} query {i}"
                cases += 1
    return cases


def link_scores(D, dtype, shape):
    """(rows uint16 [n,D] in row order, base, the oracle's score matrix [n, n] of the live rows against themselves)."""
    from tests.support import bits
    rows, _, base, _ = MR.host_dataset(D, dtype, shape)
    live = np.ascontiguousarray(bits(rows[base:]))
    return live, base, cref.cosine_matrix(live, live, dtype=dtype)


def link_precondition(D, dtype, shape) -> int:
    """The same condition for the link test: queries are the stored rows themselves, every (k, min_gap, max_back) of the
    test; -> the number of (query, parameter set) cases checked."""
    live, base, scores = link_scores(D, dtype, shape)
    n = live.shape[0]
    cases = 0
    for k in LINK_KS:
        for gap in LINK_GAPS:
            for back in LINK_BACKS:
                sel = selection(link_spans(base, n, base, gap, back), n, base, n)
                for i in range(n):
                    assert gap_ok(np.sort(scores[i][sel[i]])[::-1], D, k), \
                        f"precondition: {shape} D={D} {dtype} k={k} gap={gap} back={back} row {base + i}"
                    cases += 1
    return cases


# ---- the end-to-end test's videos -----------------------------------------------------------------------------------
E2E_D, E2E_A, E2E_B, E2E_GAP = 128, 48, 40, 16


def e2e_videos(seed=11):
    """uint16 [A + B + A, D] fp16 bit patterns: video A, video B, then A' = A's rows plus small noise.  A video is a slow
    drift (each frame the previous one plus a step), so a frame resembles its temporal neighbours most - what min_gap is
    there to keep out - and the aligned frame of the first showing next."""
    rng = np.random.default_rng(seed)

    def unit(x):
        return x / np.linalg.norm(x, axis=1, keepdims=True)

    def video(n):
        return unit(rng.standard_normal((1, E2E_D)) + np.cumsum(0.35 * rng.standard_normal((n, E2E_D)), axis=0))
    a, b = video(E2E_A), video(E2E_B)
    again = unit(a + 0.02 * rng.standard_normal(a.shape))
    return np.ascontiguousarray(np.concatenate([a, b, again]).astype(np.float16)).view(np.uint16)
