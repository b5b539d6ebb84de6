"""Test oracle of the mixed-query top-k (include/vidmem.h vm_topk_cosine_mix).

Contract: the score of row r for mixed query c is W(c, r) = sum_j w[c][j] * e_j(r) with e_j the raw reference cosine of
term j and row r (oracle.cref.cosine_matrix; 0.0 for a zero norm), the sum started at 0.0 and taken j = 0 .. J-1 left to
right, one rounding per product and one per addition.  Rows are ranked by (W desc, row id asc) over the live rows the
query's mask selects, ``W > min_score`` is a strict filter on the raw sum, the first k are kept, -1 / 0.0 padded.  The
score is stated twice over the same cosine matrix:

  (A) ``mix_scores_loop``   a Python-float loop per row: ``acc = 0.0; acc = acc + w[j] * e[j]``;
  (B) ``mix_scores``        array-wise with an explicit loop over j (never np.sum / np.dot: pairwise summation is another
                            function).

Both are ranked by tests/mask_ref.py ``masked_topk_from_scores``.  tests/test_mix_cpu.py holds them against each other;
the GPU tests compare with (A).  Also here: the cases, weight sets and the flag-0 condition of the scan test
(tests/test_mix_gpu.py), which the CPU file needs to prove the scan test's precondition without a GPU, and the data of
the end-to-end test.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import cref
from tests import mask_ref as MR
from tests.scored_ref import CS, DTS, JS, KS, NQ, W_MAX, W_MIN, rank_pair, scan_selections, slack_m, term_rows  # noqa: F401

WEIGHT_SETS = ("one", "mean", "feedback", "wide")


def weights_of(name: str, J: int):
    """The scan test's weight sets, as Python floats."""
    if name == "one":
        return [1.0] + [0.0] * (J - 1)
    if name == "mean":
        return [1.0 / J] * J
    if name == "feedback":
        return [(1.0, 1.0, -0.5)[j % 3] for j in range(J)]
    if name == "wide":
        return [(-1.0) ** j * 2.0 ** ((j % 5) - 2) for j in range(J)]
    raise KeyError(name)


def eps_mix(D: int, A: float) -> float:
    """The bound of the scanned score against W inside the domain: A (cert_eps(D) + 2^-21), A = sum |w_j|."""
    return A * (MR.cert_eps(D) + 2.0 ** -21)


def abs_sum(w) -> float:
    a = 0.0
    for x in w:
        a = a + abs(float(x))
    return a


def mix_scores_loop(e, w) -> np.ndarray:
    """(A).  e [J, n] fp64 cosines, w [J] -> W [n]."""
    e = np.asarray(e, dtype=np.float64)
    J, n = e.shape
    out = np.empty(n, dtype=np.float64)
    for r in range(n):
        acc = 0.0
        for j in range(J):
            acc = acc + float(w[j]) * float(e[j, r])
        out[r] = acc
    return out


def mix_scores(e, w) -> np.ndarray:
    """(B)."""
    e = np.asarray(e, dtype=np.float64)
    acc = np.zeros(e.shape[1], dtype=np.float64)
    for j in range(e.shape[0]):
        acc = acc + np.float64(w[j]) * e[j]
    return acc


def mix_topk(terms, weights, rows, sel, k, dtype="f16", min_score=None, base=0, scores=mix_scores_loop):
    """terms [C,J,D] and rows [n,D] (uint16 bit patterns, rows in row-id order), weights [C][J], sel bool [C,n] or None
    -> (rows [C,k] int64, scores [C,k] fp64) by statement (A) (``scores=mix_scores`` for (B))."""
    terms = np.ascontiguousarray(terms)
    C, J, D = terms.shape
    n = rows.shape[0]
    if sel is None:
        sel = np.ones((C, n), dtype=bool)
    W = np.zeros((C, n), dtype=np.float64)
    if n:
        e = cref.cosine_matrix(terms.reshape(C * J, D), np.ascontiguousarray(rows), dtype=dtype).reshape(C, J, n)
        for c in range(C):
            W[c] = scores(e[c], weights[c])
    return MR.masked_topk_from_scores(W, sel, k, min_score=min_score, base=base)


# ---- the scan test's cases --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scan_scores(D, dtype, shape, J, wname):
    """W [3, live rows] of the three mixed queries of (J, weight set) on the tile-scan dataset, by (A), from the shared
    oracle matrix; the weights [J]."""
    _, _, _, live = MR.host_dataset(D, dtype, shape)
    w = weights_of(wname, J)
    return np.stack([mix_scores_loop(live[term_rows(c, J)], w) for c in range(max(CS))]), w


def flag0_ok(best_first, k: int, D: int, A: float) -> bool:
    """best_first: one query's exact selected W, descending.  True when rank k and rank M + 1 are more than
    4 x eps_mix(D, A) apart, or when there is no rank M + 1 (everything is re-scored exactly): the fast path must then
    certify the query."""
    pair = rank_pair(best_first, k)
    return pair is None or bool(pair[0] - pair[1] > 4 * eps_mix(D, A))


def margin(best_first, k: int, D: int, A: float) -> float:
    """(rank k - rank M + 1) / eps_mix, inf when there is no rank M + 1."""
    pair = rank_pair(best_first, k)
    return np.inf if pair is None else float((pair[0] - pair[1]) / eps_mix(D, A))


# ---- the end-to-end test's data ---------------------------------------------------------------------------------------
E2E_D, E2E_N = 128, 60


def e2e_videos(seed=23):
    """uint16 [2 N, D] fp16 bit patterns: two "videos" of N frames in the manner of span_ref.e2e_videos - each a slow
    drift, so a frame resembles its temporal neighbours most."""
    rng = np.random.default_rng(seed)

    def video(n):
        x = rng.standard_normal((1, E2E_D)) + np.cumsum(0.35 * rng.standard_normal((n, E2E_D)), axis=0)
        return x / np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(np.concatenate([video(E2E_N), video(E2E_N)]).astype(np.float16)).view(np.uint16)
