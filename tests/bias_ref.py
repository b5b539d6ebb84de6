"""Test oracle of the biased top-k (include/vidmem.h vm_topk_cosine_biased).

Contract: a bias column holds one fp32 value per physical slot, the entry of row id r being entry r mod capacity; entries
of slots without a live row are ignored.  The score of row r for query q is S(q, r) = e(q, r) + beta_q * b[slot(r)] with e
the raw reference cosine (oracle.cref.cosine_matrix; 0.0 for a zero norm), b widened exactly to fp64, one rounding for
the product and one for the sum.  Rows are ranked by (S desc, row id asc) over the live rows the query's mask selects,
``S > min_score`` is a strict filter on the raw sum, the first k are kept, -1 / 0.0 padded.  The score is stated twice
over the same cosine matrix:

  (A) ``bias_scores_loop``   a Python-float loop per row: ``float(e) + float(beta) * float(b)``;
  (B) ``bias_scores``        array-wise numpy in fp64.

Both are ranked by tests/mask_ref.py ``masked_topk_from_scores``.  tests/test_bias_cpu.py holds them against each other;
the GPU tests compare with (A).  Also here: the bias sets, the weights and the flag-0 condition of the scan test
(tests/test_bias_gpu.py), which the CPU file needs to prove the scan test's precondition without a GPU, the restatements
of the two device-side builders, and the data of the end-to-end test.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import cref
from tests import mask_ref as MR
from tests import mix_ref as XR
from tests.scored_ref import DTS, NQ, rank_pair, scan_selections, slack_m  # noqa: F401

QS = (1, 17, 33)                    # QT = 1, QT = 2 with a ragged second tile, and a second query group
KS = (1, 5)
SETS = ("zero", "age", "boost", "wide", "big")
BETAS = (1.0, 0.0, -0.5, 0.3, 2.0 ** -12)
W_MIN, W_MAX, B_MAX = 2.0 ** -20, 2.0 ** 20, 2.0 ** 40      # the domain of the bound: |beta| (or 0), and |b|
TAG_MS_MASK = (1 << 40) - 1
INT64_MIN = -(1 << 63)


def bias_stride(capacity: int) -> int:
    """S: the entries of one column, the capacity rounded up to 64 (= 32 x mask_ref.mask_words)."""
    return (capacity + 63) // 64 * 64


def eps_bias(D: int, B: float) -> float:
    """The bound of the scanned score B against S inside the domain: cert_eps(D) + 2^-21 + 2^-22 |B|."""
    return MR.cert_eps(D) + 2.0 ** -21 + 2.0 ** -22 * abs(float(B))


# ---- the score, twice -------------------------------------------------------------------------------------------------
def bias_scores_loop(e, beta, b) -> np.ndarray:
    """(A).  e [n] fp64 cosines, beta one weight, b [n] fp32 bias values of the same rows -> S [n]."""
    out = np.empty(len(e), dtype=np.float64)
    for r in range(len(e)):
        out[r] = float(e[r]) + float(beta) * float(b[r])
    return out


def bias_scores(e, beta, b) -> np.ndarray:
    """(B)."""
    return np.asarray(e, dtype=np.float64) + np.float64(beta) * np.asarray(b, dtype=np.float32).astype(np.float64)


def row_bias(cols, bias_index, Q: int, base: int, n: int, capacity: int) -> np.ndarray:
    """fp32 [Q, n]: the bias value of every live row base .. base + n - 1 for every query, by vm_topk_cosine_biased's
    rule: entry r mod capacity of the query's column; no index = column 0 for all (one column) or column q (Q columns);
    an index outside [0, n_bias) = the zero column."""
    cols = np.asarray(cols, dtype=np.float32).reshape(-1, bias_stride(capacity))
    if bias_index is None:
        assert cols.shape[0] in (1, Q)
        bias_index = [0] * Q if cols.shape[0] == 1 else list(range(Q))
    slots = (base + np.arange(n, dtype=np.int64)) % capacity
    out = np.zeros((Q, n), dtype=np.float32)
    for q, i in enumerate(bias_index):
        if 0 <= int(i) < cols.shape[0]:
            out[q] = cols[int(i)][slots]
    return out


def bias_topk_from_cosines(e, betas, b, sel, k, min_score=None, base=0, scores=bias_scores_loop):
    """e [Q, n] cosines, betas [Q], b fp32 [Q, n], sel bool [Q, n] or None -> (rows [Q,k] int64, scores [Q,k] fp64)."""
    Q, n = e.shape
    if sel is None:
        sel = np.ones((Q, n), dtype=bool)
    S = np.zeros((Q, n), dtype=np.float64)
    for q in range(Q):
        S[q] = scores(e[q], betas[q], b[q])
    return MR.masked_topk_from_scores(S, sel, k, min_score=min_score, base=base)


def bias_topk(queries, rows, cols, bias_index, betas, sel, k, dtype="f16", min_score=None, base=0, capacity=None,
              scores=bias_scores_loop):
    """queries [Q,D] and rows [n,D] (uint16 bit patterns, rows in row-id order from ``base``), cols fp32 [n_bias, S],
    betas [Q] (None: 1.0), sel bool [Q,n] or None -> (rows [Q,k] int64, scores [Q,k] fp64) by statement (A)
    (``scores=bias_scores`` for (B))."""
    queries = np.ascontiguousarray(queries)
    Q, n = queries.shape[0], rows.shape[0]
    capacity = capacity or max(n, 1)
    betas = [1.0] * Q if betas is None else list(betas)
    e = cref.cosine_matrix(queries, np.ascontiguousarray(rows), dtype=dtype) if n else np.zeros((Q, 0))
    return bias_topk_from_cosines(e, betas, row_bias(cols, bias_index, Q, base, n, capacity), sel, k, min_score, base,
                                  scores)


# ---- the scan test's cases --------------------------------------------------------------------------------------------
def set_value(name: str, r: int, base: int, n: int) -> float:
    """The bias of row id r of the n live rows from ``base``; every value is exactly an fp32."""
    if name == "zero":
        return 0.0
    if name == "age":
        return -(base + n - 1 - r) / 64.0
    if name == "boost":
        return 0.5 if r % 7 == 3 else 0.0
    if name == "wide":
        return (-1.0) ** r * 2.0 ** ((r % 5) - 2)
    if name == "big":
        return (1000.0 if r % 11 == 5 else -3.0) + 0.125 * (r % 4)
    raise KeyError(name)


def set_columns(base: int, n: int, capacity: int, dead=np.nan) -> np.ndarray:
    """fp32 [5, S]: the five sets as columns of a memory whose live rows are base .. base + n - 1.  Slots without a live
    row hold ``dead`` (NaN: every consumer must ignore them)."""
    cols = np.full((len(SETS), bias_stride(capacity)), dead, dtype=np.float32)
    for i, name in enumerate(SETS):
        for r in range(base, base + n):
            v = set_value(name, r, base, n)
            assert float(np.float32(v)) == v, (name, r)
            cols[i, r % capacity] = v
    return cols


def query_case(i: int):
    """(set index, weight) of query i of the scan test: every (set, weight) pair occurs among the first 25 queries."""
    return (i // 5) % 5, BETAS[i % 5]


def flag0_ok(best_first, k: int, D: int) -> bool:
    """best_first: one query's exact selected S, descending.  True when rank k and rank M + 1 are more than
    4 x eps_bias apart - the bound taken at the larger magnitude of the two -, or when there is no rank M + 1 (everything
    is re-scored exactly): the fast path must then certify the query.  Why 4 suffices: B - eps_bias(B) is increasing and
    at most S, so the (M+1)-th scanned score B* is at most rank M + 1 + eps_bias; a row whose S is at least rank k has a
    scanned score of at least rank k - eps_bias > B*, so the k best rows are among the M re-scored ones and the exact
    k-th is rank k, which clears B* + eps_bias(B*) when the two ranks are more than 2 (1 + 2^-21) eps_bias apart."""
    return margin(best_first, k, D) > 4


def margin(best_first, k: int, D: int) -> float:
    """(rank k - rank M + 1) / eps_bias, inf when there is no rank M + 1."""
    pair = rank_pair(best_first, k)
    if pair is None:
        return np.inf
    hi, lo = float(pair[0]), float(pair[1])
    return (hi - lo) / eps_bias(D, max(abs(hi), abs(lo)))


@functools.lru_cache(maxsize=None)
def scan_scores(D, dtype, shape):
    """S [5 sets][5 weights] -> [33, live rows] by (A) over the tile-scan dataset's shared cosine matrix."""
    _, _, base, live = MR.host_dataset(D, dtype, shape)
    total, cap = MR.SHAPES[shape]
    n = live.shape[1]
    cols = set_columns(base, n, cap or total)
    out = {}
    for si in range(len(SETS)):
        b = row_bias(cols[si:si + 1], None, 1, base, n, cap or total)[0]
        for beta in BETAS:
            out[si, beta] = np.stack([bias_scores_loop(live[q], beta, b) for q in range(NQ)])
    return out


# ---- the builders, restated --------------------------------------------------------------------------------------------
def bias_from_rows_ref(row_ids, values, base: int, n: int, capacity: int, start=None, stride=(1, 0)) -> np.ndarray:
    """vm_bias_from_rows: fp32 [S].  ``start``: the column before the call (clear_first == 0), default zeros.  The test's
    duplicates carry one value, so the order of the stores does not matter here."""
    col = np.zeros(bias_stride(capacity), dtype=np.float32) if start is None else np.array(start, dtype=np.float32)
    for rid, v in zip(row_ids, values):
        d = int(rid) - stride[1]
        if int(rid) < 0 or d < 0 or d % stride[0]:
            continue
        r = d // stride[0]
        if base <= r < base + n:
            col[r % capacity] = np.float32(v)
    return col


def bias_from_tags_ref(tags, base: int, capacity: int, t_ref_ms: int, per_ms: float, fill: float) -> np.ndarray:
    """vm_bias_from_tags: fp32 [S] from the tags of the live rows in row-id order from ``base``: per_ms * d with one fp64
    rounding, d = (tag & (2^40 - 1)) - t_ref_ms exact, then round to nearest even to fp32; ``fill`` for untagged rows and
    for slots without a live row."""
    col = np.full(bias_stride(capacity), np.float32(fill), dtype=np.float32)
    for i, t in enumerate(tags):
        t = int(t)
        if t != INT64_MIN:
            d = (t & TAG_MS_MASK) - int(t_ref_ms)
            assert float(d) == d and abs(d) < 2 ** 53
            col[(base + i) % capacity] = np.float32(float(per_ms) * float(d))
    return col


# ---- the end-to-end test's data ---------------------------------------------------------------------------------------
E2E_D, E2E_N, E2E_FRAME_MS = 128, 60, 1000


def e2e_videos(seed=29):
    """uint16 [2 N, D] fp16 bit patterns: two "videos" of N frames, each a slow drift, so a frame resembles its temporal
    neighbours most: mix_ref.e2e_videos with another seed."""
    assert (E2E_D, E2E_N) == (XR.E2E_D, XR.E2E_N)
    return XR.e2e_videos(seed)


def e2e_tags() -> np.ndarray:
    """int64 [2 N]: video v, frame i is tagged (v << 40) | (i * 1000 ms); the two videos cover the same minute."""
    return np.array([(v << 40) | (i * E2E_FRAME_MS) for v in range(2) for i in range(E2E_N)], dtype=np.int64)
