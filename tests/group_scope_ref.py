"""Test oracle of the scoped grouped top-k (include/vidmem.h vm_topk_cosine_grouped_scoped).

Contract: the exhaustive row ranking of vm_topk_cosine_scoped - raw reference cosines (oracle.cref.cosine_matrix) of the
rows whose tag lies in the query's inclusive range [lo, hi] (tests/scope_ref.py scope_mask), ranked by (raw score desc,
row id asc), the score_mode mapping, the strict ``> min_score`` filter on the mapped score - with only the first row of
each group kept, then the first k; -1 / 0.0 / -1 padded.  Groups are runs of equal consecutive keys over ALL rows
(tests/group_ref.py group_ids): a scope hides rows, it neither splits a group around a hidden row nor merges the two
neighbours of a hidden group, and a group with no in-scope row does not exist for the query.

Two statements: ``group_scoped_topk_from_scores`` (vectorised: mask, rank, first row per group) and
``group_scoped_topk_py`` (plain loops: per group the raw max over its in-scope rows and the lowest row reaching it).
tests/test_group_scope_cpu.py holds them against each other; the GPU tests compare with the first.
"""
from __future__ import annotations

import numpy as np

from oracle import cref
from tests.group_ref import group_ids
from tests.scope_ref import scope_arrays, scope_mask


def group_scoped_topk_from_scores(scores, keys, tags, scopes, k, score_mode=0, min_score=None, base=0):
    """scores [Q,n] raw fp64 cosines, keys [n], tags [n] in row-id order; scopes: one (lo, hi) or Q pairs ->
    (rows [Q,k] int64, scores [Q,k] fp64, keys [Q,k] int64); rows = base + row index."""
    scores = np.asarray(scores, dtype=np.float64)
    keys = np.asarray(keys, dtype=np.int64)
    Q, n = scores.shape
    lo, hi = scope_arrays(scopes, Q)
    gid = group_ids(keys)                                   # over all rows: a scope does not redefine groups
    out_r = np.full((Q, k), -1, np.int64)
    out_s = np.zeros((Q, k), np.float64)
    out_k = np.full((Q, k), -1, np.int64)
    for q in range(Q):
        raw = scores[q]
        shown = (1.0 + raw) / 2.0 if score_mode == 1 else raw
        keep = scope_mask(tags, lo[q], hi[q])
        if min_score is not None:
            keep &= shown > min_score
        cand = np.nonzero(keep)[0]
        order = cand[np.lexsort((cand, -raw[cand]))]        # raw score desc, row asc
        _, first = np.unique(gid[order], return_index=True)
        best = order[np.sort(first)][:k]                    # first row of each group, in ranking order
        out_r[q, :best.size] = base + best
        out_s[q, :best.size] = shown[best]
        out_k[q, :best.size] = keys[best]
    return out_r, out_s, out_k


def group_scoped_topk(queries, rows, keys, tags, scopes, k, dtype="f16", score_mode=0, min_score=None, base=0):
    """queries [Q,D], rows [n,D] (uint16 bit patterns), keys / tags [n] in row-id order."""
    return group_scoped_topk_from_scores(cref.cosine_matrix(queries, rows, dtype=dtype), keys, tags, scopes, k,
                                         score_mode, min_score, base)


def group_scoped_topk_py(scores, keys, tags, scopes, k, score_mode=0, min_score=None, base=0):
    """Plain-loop restatement: walk the rows once; a key change opens a group whether or not the row is in scope; a
    group collects the raw max over its in-scope rows and the lowest row reaching it; a group that collected nothing is
    dropped; groups by (max desc, row asc); the mapping and the filter applied to each group's max."""
    Q = len(scores)
    lo, hi = scope_arrays(scopes, Q)
    out_r = [[-1] * k for _ in range(Q)]
    out_s = [[0.0] * k for _ in range(Q)]
    out_k = [[-1] * k for _ in range(Q)]
    for q in range(Q):
        groups, prev = [], None
        for i, (sv, key, tag) in enumerate(zip(scores[q], keys, tags)):
            if i == 0 or key != prev:
                groups.append([None, None, int(key)])
            prev = key
            if not (int(lo[q]) <= int(tag) <= int(hi[q])):
                continue
            g, sv = groups[-1], float(sv)
            if g[0] is None or sv > g[0]:
                g[0], g[1] = sv, i
        seen = [g for g in groups if g[0] is not None]
        shown = [((1.0 + g[0]) / 2.0 if score_mode == 1 else g[0], g) for g in seen]
        live = [(m, g) for m, g in shown if min_score is None or m > min_score]
        live.sort(key=lambda mg: (-mg[1][0], mg[1][1]))
        for j, (m, g) in enumerate(live[:k]):
            out_r[q][j], out_s[q][j], out_k[q][j] = base + g[1], m, g[2]
    return np.array(out_r, np.int64), np.array(out_s, np.float64), np.array(out_k, np.int64)
