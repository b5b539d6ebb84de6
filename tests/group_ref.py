"""Test oracle of the grouped top-k (include/vidmem.h vm_topk_cosine_grouped).

Contract: the exhaustive row ranking of vm_topk_cosine - oracle.cref.cosine_matrix (the exact C restatement of the
reference cosine), a stable sort of the RAW scores by (score desc, row id asc), the ``> min_score`` filter on the mapped
score - with only the first row of each group kept, then the first k, mapped.  A group is a maximal run of consecutive
rows with equal keys.  Ranking the raw scores and mapping afterwards is what the kernels do (as vm_topk_cosine does):
two raw scores one ulp apart that (1 + s) / 2 maps to one value keep their raw order.
``grouped_topk_py`` restates the same contract in plain Python loops (the check of the vectorised version).
"""
from __future__ import annotations

import numpy as np

from oracle import cref


def group_ids(keys) -> np.ndarray:
    """Group index of every row: runs of equal consecutive keys (a key that comes back opens a new group)."""
    keys = np.asarray(keys, dtype=np.int64)
    if keys.size == 0:
        return np.zeros(0, np.int64)
    return np.concatenate([[0], np.cumsum(keys[1:] != keys[:-1])]).astype(np.int64)


def _mapped(scores: np.ndarray, score_mode: int) -> np.ndarray:
    return (1.0 + scores) / 2.0 if score_mode == 1 else scores


def grouped_topk_from_scores(scores, keys, k, score_mode=0, min_score=None, base=0):
    """scores [Q,n] fp64 (row-id order), keys [n] -> (rows [Q,k] int64, scores [Q,k] fp64, keys [Q,k] int64), -1 / 0.0
    / -1 padded; rows = base + row index."""
    scores = np.asarray(scores, dtype=np.float64)
    keys = np.asarray(keys, dtype=np.int64)
    Q, n = scores.shape
    gid = group_ids(keys)
    out_r = np.full((Q, k), -1, np.int64)
    out_s = np.zeros((Q, k), np.float64)
    out_k = np.full((Q, k), -1, np.int64)
    idx = np.arange(n, dtype=np.int64)
    for q in range(Q):
        raw = scores[q]
        s = _mapped(raw, score_mode)
        keep = np.ones(n, bool) if min_score is None else s > min_score
        cand = idx[keep]
        order = cand[np.lexsort((cand, -raw[cand]))]    # raw score desc, row asc
        _, first = np.unique(gid[order], return_index=True)
        best = order[np.sort(first)][:k]                 # first row of each group, in ranking order
        m = best.size
        out_r[q, :m] = base + best
        out_s[q, :m] = s[best]
        out_k[q, :m] = keys[best]
    return out_r, out_s, out_k


def grouped_topk(queries, rows, keys, k, dtype="f16", score_mode=0, min_score=None, base=0):
    """queries [Q,D], rows [n,D] (uint16 bit patterns or float16), keys [n] in row-id order."""
    return grouped_topk_from_scores(cref.cosine_matrix(queries, rows, dtype=dtype), keys, k, score_mode, min_score,
                                    base)


def grouped_topk_py(scores, keys, k, score_mode=0, min_score=None, base=0):
    """Plain-loop restatement: per group, the raw max and the lowest row reaching it; groups by (max desc, row asc);
    the mapping and the filter applied to each group's max."""
    Q = len(scores)
    out_r = [[-1] * k for _ in range(Q)]
    out_s = [[0.0] * k for _ in range(Q)]
    out_k = [[-1] * k for _ in range(Q)]
    for q in range(Q):
        groups = []  # [best score, best row, key] of each run
        prev = None
        for i, (sv, key) in enumerate(zip(scores[q], keys)):
            sv = float(sv)
            if i == 0 or key != prev:
                groups.append([None, None, int(key)])
            prev = key
            g = groups[-1]
            if g[0] is None or sv > g[0]:
                g[0], g[1] = sv, i
        shown = [((1.0 + g[0]) / 2.0 if score_mode == 1 else g[0], g) for g in groups]
        live = [(m, g) for m, g in shown if min_score is None or m > min_score]
        live.sort(key=lambda mg: (-mg[1][0], mg[1][1]))
        for j, (m, g) in enumerate(live[:k]):
            out_r[q][j], out_s[q][j], out_k[q][j] = base + g[1], m, g[2]
    return np.array(out_r, np.int64), np.array(out_s, np.float64), np.array(out_k, np.int64)
