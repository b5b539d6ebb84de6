"""Test oracle of the scoped top-k (include/vidmem.h vm_topk_cosine_scoped).

Contract: row r is in query q's scope iff lo[q] <= tag[r] <= hi[q]; the result is the exhaustive row ranking of
vm_topk_cosine - raw reference cosines ranked by (score desc, row id asc), the score_mode mapping, the ``> min_score``
filter on the mapped score - taken over the in-scope rows only, first k; -1 / 0.0 padded.  Two independent statements:

  (A) ``scoped_topk``        oracle.cref.cosine_topk (the C restatement of the reference ranking) on the in-scope rows
                             only, its indices mapped back to row ids: ascending index order keeps the stable tie rule;
  (B) ``scoped_topk_matrix`` oracle.cref.cosine_matrix over all rows, masked, the raw scores ranked by
                             (score desc, row asc), then mapped and filtered.

tests/test_scope_cpu.py holds them against each other; the GPU tests compare with (A).
"""
from __future__ import annotations

import numpy as np

from oracle import cref

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def scope_arrays(scopes, Q):
    """One (lo, hi) for all queries, or Q pairs -> (lo [Q], hi [Q]) int64."""
    sc = np.asarray(scopes, dtype=np.int64)
    if sc.ndim == 1:
        sc = np.tile(sc, (Q, 1))
    assert sc.shape == (Q, 2), sc.shape
    return sc[:, 0].copy(), sc[:, 1].copy()


def scope_mask(tags, lo, hi) -> np.ndarray:
    tags = np.asarray(tags, dtype=np.int64)
    return (tags >= lo) & (tags <= hi)


def scoped_topk(queries, rows, tags, scopes, k, dtype="f16", score_mode=0, min_score=None, base=0):
    """(A).  queries [Q,D], rows [n,D] (uint16 bit patterns), tags [n] in row-id order -> (rows [Q,k] int64,
    scores [Q,k] fp64); rows = base + row index."""
    queries = np.ascontiguousarray(queries)
    rows = np.ascontiguousarray(rows)
    Q = queries.shape[0]
    lo, hi = scope_arrays(scopes, Q)
    out_r = np.full((Q, k), -1, np.int64)
    out_s = np.zeros((Q, k), np.float64)
    pairs = {}
    for q in range(Q):
        pairs.setdefault((int(lo[q]), int(hi[q])), []).append(q)
    for (l, h), qs in pairs.items():       # queries of one scope share one restricted memory
        idx = np.nonzero(scope_mask(tags, l, h))[0]
        if idx.size == 0:
            continue
        r, s = cref.cosine_topk(queries[qs], rows[idx], k, dtype=dtype, score_mode=score_mode, min_score=min_score)
        out_r[qs] = np.where(r >= 0, base + idx[np.maximum(r, 0)], -1)
        out_s[qs] = s
    return out_r, out_s


def scoped_topk_from_scores(scores, tags, scopes, k, score_mode=0, min_score=None, base=0):
    """scores [Q,n] raw fp64 cosines in row-id order -> the masked ranking."""
    scores = np.asarray(scores, dtype=np.float64)
    Q, n = scores.shape
    lo, hi = scope_arrays(scopes, Q)
    out_r = np.full((Q, k), -1, np.int64)
    out_s = np.zeros((Q, k), np.float64)
    for q in range(Q):
        raw = scores[q]
        shown = (1.0 + raw) / 2.0 if score_mode == 1 else raw
        keep = scope_mask(tags, lo[q], hi[q])
        if min_score is not None:
            keep &= shown > min_score
        cand = np.nonzero(keep)[0]
        best = cand[np.lexsort((cand, -raw[cand]))][:k]     # raw score desc, row asc
        out_r[q, :best.size] = base + best
        out_s[q, :best.size] = shown[best]
    return out_r, out_s


def scoped_topk_matrix(queries, rows, tags, scopes, k, dtype="f16", score_mode=0, min_score=None, base=0):
    """(B)."""
    return scoped_topk_from_scores(cref.cosine_matrix(queries, rows, dtype=dtype), tags, scopes, k, score_mode,
                                   min_score, base)
