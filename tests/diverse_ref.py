"""Test oracle of the diverse top-k (include/vidmem.h vm_topk_cosine_diverse).

Contract: the POOL of a query is the exhaustive ranking of vm_topk_cosine over the live rows its mask selects, after the
strict ``e > min_score`` filter, first ``pool`` entries: rows r_0 .. r_{np-1} ordered (e desc, row id asc).  With
``mu = 1.0 - lam`` and ``sim(i, j)`` the reference cosine between stored rows r_i and r_j (oracle.cref.cosine_matrix of the
rows with themselves; 0.0 for a zero norm), step 0 takes r_0 and every later step takes the unpicked i with the largest
``v_i = lam * e_i - mu * red_i``, ``red_i`` the maximum (plain >, from 0.0) of sim(i, s) over the picked s, ties to the
smaller row id; every operation is one fp64 rounding.  min(k, np) picks; outputs in pick order: row ids, relevance e and
the v of each pick, -1 / 0.0 / 0.0 padded.  Stated twice over oracle.cref:

  (A) ``diverse_topk``        a Python-float loop over the pool of cref.cosine_topk (tests/mask_ref.py masked_topk under a
                              mask) and cref.cosine_matrix(rows, rows);
  (B) ``diverse_topk_arrays`` the pool from mask_ref.masked_topk_from_scores over the oracle's score matrix, one numpy
                              statement per step, ``np.maximum`` for red (never np.dot / np.sum on scores).

tests/test_diverse_cpu.py holds them against each other; the GPU tests compare with (A).  Also here: the cases of the GPU
scan test and its two preconditions, which the CPU file proves without a GPU, and the data of the end-to-end test.
"""
from __future__ import annotations

import numpy as np

from oracle import cref
from tests import mask_ref as MR
from tests import scored_ref
from tests.scored_ref import DTS, rank_pair, slack_m  # noqa: F401

QS = (1, 16, 17, 33)
K_POOL = ((1, 1), (5, 5), (5, 8), (5, 16), (5, 64), (17, 33), (64, 64))
POOLS = (5, 8, 16, 64)              # the pools of precondition (i)
LAMS = (0.0, 0.5, 0.7, 1.0)


def lam_vector(Q: int):
    """The scan test's per-query lam: a different value of [0, 1] for neighbouring queries."""
    return [(0.0, 0.3, 0.5, 0.7, 1.0, 0.9)[i % 6] for i in range(Q)]


def per_query(lam, Q: int):
    return [float(x) for x in lam] if hasattr(lam, "__len__") else [float(lam)] * Q


def sim_matrix(rows, dtype="f16") -> np.ndarray:
    """sim [n, n] of stored rows (uint16 bit patterns): the reference cosine of each pair."""
    rows = np.ascontiguousarray(rows)
    if rows.shape[0] == 0:
        return np.zeros((0, 0), dtype=np.float64)
    return cref.cosine_matrix(rows, rows, dtype=dtype)


def greedy_loop(ids, e, sim, k: int, lam: float):
    """(A)'s pick.  ids [np] row ids, e [np] their relevance (pool order), sim [np, np] -> (picked pool indices, v of each
    pick), Python floats throughout."""
    n = len(ids)
    lam = float(lam)
    mu = 1.0 - lam
    red = [0.0] * n
    open_ = [True] * n
    picks, vals = [], []
    for t in range(min(k, n)):
        if t == 0:
            w, vw = 0, lam * float(e[0]) - mu * 0.0
        else:
            w, vw = -1, 0.0
            for i in range(n):
                if not open_[i]:
                    continue
                v = lam * float(e[i]) - mu * red[i]
                if w < 0 or v > vw or (v == vw and int(ids[i]) < int(ids[w])):
                    w, vw = i, v
        picks.append(w)
        vals.append(vw)
        open_[w] = False
        for i in range(n):
            s = float(sim[i, w])
            if s > red[i]:
                red[i] = s
    return picks, vals


def greedy_arrays(ids, e, sim, k: int, lam: float):
    """(B)'s pick: one array statement per step."""
    ids = np.asarray(ids, dtype=np.int64)
    e = np.asarray(e, dtype=np.float64)
    n = ids.size
    lam = np.float64(lam)
    mu = np.float64(1.0) - lam
    red = np.zeros(n, dtype=np.float64)
    open_ = np.ones(n, dtype=bool)
    picks, vals = [], []
    for t in range(min(k, n)):
        v = lam * e - mu * red
        if t == 0:
            w = 0
        else:
            cand = np.nonzero(open_)[0]
            w = int(cand[np.lexsort((ids[cand], -v[cand]))][0])     # v desc, row id asc
        picks.append(w)
        vals.append(float(v[w]))
        open_[w] = False
        red = np.maximum(red, sim[w])                               # sim is bit-symmetric: row w = column w
    return picks, vals


def _pick_all(pool_r, pool_s, rows, k, lam, dtype, base, greedy, sim=None):
    """``sim``: sim_matrix(rows) when the caller has it (the same function over all rows at once)."""
    Q = pool_r.shape[0]
    lams = per_query(lam, Q)
    out_r = np.full((Q, k), -1, np.int64)
    out_s = np.zeros((Q, k), np.float64)
    out_v = np.zeros((Q, k), np.float64)
    for q in range(Q):
        ids = pool_r[q][pool_r[q] >= 0]
        if ids.size == 0:
            continue
        e = pool_s[q][:ids.size]
        at = ids - base
        picks, vals = greedy(ids, e, sim_matrix(rows[at], dtype) if sim is None else sim[np.ix_(at, at)], k, lams[q])
        out_r[q, :len(picks)] = ids[picks]
        out_s[q, :len(picks)] = e[picks]
        out_v[q, :len(picks)] = vals
    return out_r, out_s, out_v


def diverse_topk(queries, rows, sel, k, pool, lam, dtype="f16", min_score=None, base=0, sim=None):
    """(A).  queries [Q,D] and rows [n,D] (uint16 bit patterns, rows in row-id order), sel bool [Q,n] or None, lam one
    float or Q of them -> (rows [Q,k] int64, scores [Q,k] fp64, mmr [Q,k] fp64) in pick order."""
    queries, rows = np.ascontiguousarray(queries), np.ascontiguousarray(rows)
    Q, n = queries.shape[0], rows.shape[0]
    if sel is None:
        sel = np.ones((Q, n), dtype=bool)
    pool_r, pool_s = MR.masked_topk(queries, rows, sel, pool, dtype=dtype, min_score=min_score, base=base)
    return _pick_all(pool_r, pool_s, rows, k, lam, dtype, base, greedy_loop, sim)


def diverse_topk_arrays(queries, rows, sel, k, pool, lam, dtype="f16", min_score=None, base=0, scores=None, sim=None):
    """(B).  ``scores``: the oracle's matrix [Q, n] when the caller has it."""
    queries, rows = np.ascontiguousarray(queries), np.ascontiguousarray(rows)
    Q, n = queries.shape[0], rows.shape[0]
    if sel is None:
        sel = np.ones((Q, n), dtype=bool)
    if scores is None:
        scores = cref.cosine_matrix(queries, rows, dtype=dtype) if n else np.zeros((Q, 0))
    pool_r, pool_s = MR.masked_topk_from_scores(scores, sel, pool, min_score=min_score, base=base)
    return _pick_all(pool_r, pool_s, rows, k, lam, dtype, base, greedy_arrays, sim)


# ---- the scan test's cases and preconditions ------------------------------------------------------------------------------
def scan_selections(Q, shape, base, n):
    """name -> (masks, index, bool [Q, n]): 'none' (no mask) and every set of mask_ref.mask_sets."""
    operands = {"none": (None, None), **MR.mask_sets(Q, shape)}
    return {name: (*operands[name], sel) for name, sel in scored_ref.scan_selections(Q, shape, base, n).items()}


def flag0_ok(best_first, pool: int, D: int) -> bool:
    """best_first: one query's exact selected scores, descending.  True when the pool search (k = pool) must certify the
    query itself: rank ``pool`` and rank M + 1 are more than 4 x cert_eps(D) apart, or fewer than M + 1 rows are
    selected."""
    pair = rank_pair(best_first, pool)
    return pair is None or bool(pair[0] - pair[1] > 4 * MR.cert_eps(D))


# ---- the end-to-end test's data -------------------------------------------------------------------------------------------
E2E_D, E2E_SCENES, E2E_K = 128, 6, 5


def e2e_videos(seed=29):
    """-> (uint16 [n, D] fp16 bit patterns, scene of each row [n], video of each row [n]).  Two "videos" cut from the same
    E2E_SCENES scenes, 3 frames per shot with small noise: scene 0 - a static camera - is shown twice in each video, every
    other scene once, and every other scene resembles scene 0 somewhat.  Plain top-5 for a view of scene 0 returns five of
    its 12 frames."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((E2E_SCENES, E2E_D))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    centres[1:] = 0.6 * centres[0] + 0.8 * centres[1:]
    rows, scene, video = [], [], []
    for v in range(2):
        for s in (0, 1, 2, 0, 3, 4, 5):
            for _ in range(3):
                x = centres[s] + 0.02 * rng.standard_normal(E2E_D)
                rows.append(x / np.linalg.norm(x))
                scene.append(s)
                video.append(v)
    bits = np.ascontiguousarray(np.array(rows).astype(np.float16)).view(np.uint16)
    return bits, np.array(scene), np.array(video)


def e2e_queries(seed=30, n=3):
    """fp16 bit patterns [n, D]: views of scene 0."""
    rng = np.random.default_rng(seed)
    bits, scene, _ = e2e_videos()
    c = bits[scene == 0][0].view(np.float16).astype(np.float64)
    q = c[None] + 0.03 * rng.standard_normal((n, E2E_D))
    return np.ascontiguousarray(q.astype(np.float16)).view(np.uint16)
