"""Test oracle of the range search (include/vidmem.h vm_range_cosine).

Contract: for query q a hit is a row r in q's scope (lo[q] <= tag[r] <= hi[q]; no scopes = every row) whose shown score
- the raw reference cosine under the score_mode mapping - is STRICTLY above min_score.  The hits come in ascending row
id with the full count.  Scores are oracle.cref.cosine_matrix's (the C restatement of the reference cosine); the mapping
and the strict ``>`` are written as tests/scope_ref.py writes them.
"""
from __future__ import annotations

import numpy as np

from oracle import cref
from tests.domain_ref import cert_eps  # noqa: F401  (the fp32 scan's error bound on a cosine; R.cert_eps for the tests)
from tests.scope_ref import scope_arrays, scope_mask

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def shown(raw, score_mode=0):
    raw = np.asarray(raw, dtype=np.float64)
    return (1.0 + raw) / 2.0 if score_mode == 1 else raw


def range_from_scores(scores, min_score, tags=None, scopes=None, score_mode=0, base=0):
    """scores [Q, n] raw fp64 cosines in row-id order -> per query (rows int64 ascending, shown scores fp64, count)."""
    scores = np.asarray(scores, dtype=np.float64)
    Q, n = scores.shape
    lo = hi = None
    if scopes is not None:
        lo, hi = scope_arrays(scopes, Q)
    out = []
    for q in range(Q):
        sh = shown(scores[q], score_mode)
        keep = sh > min_score
        if scopes is not None:
            keep &= scope_mask(tags, lo[q], hi[q])
        idx = np.nonzero(keep)[0].astype(np.int64)
        out.append((base + idx, sh[idx], int(idx.size)))
    return out


def range_hits(queries, rows, min_score, tags=None, scopes=None, dtype="f16", score_mode=0, base=0):
    """queries [Q, D], rows [n, D] (uint16 bit patterns), tags [n] in row-id order."""
    m = cref.cosine_matrix(np.ascontiguousarray(queries), np.ascontiguousarray(rows), dtype=dtype)
    return range_from_scores(m, min_score, tags, scopes, score_mode, base)


def padded(hits, max_hits):
    """The [Q, max_hits] arrays the C entry writes: the first max_hits hits, -1 / 0.0 padded, and the full counts."""
    Q = len(hits)
    rows = np.full((Q, max_hits), -1, np.int64)
    scores = np.zeros((Q, max_hits), np.float64)
    counts = np.zeros(Q, np.int64)
    for q, (r, s, c) in enumerate(hits):
        w = min(c, max_hits)
        rows[q, :w] = r[:w]
        scores[q, :w] = s[:w]
        counts[q] = c
    return rows, scores, counts
