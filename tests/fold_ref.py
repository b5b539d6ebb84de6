"""Test oracle of the any/all top-k (include/vidmem.h vm_topk_cosine_fold).

Contract: for fold query c with terms t_0 .. t_{J-1}, fp64 weights w_j and op in {max, min}

    p_j = fl64(w_j * e_j(r))        e_j = the raw reference cosine of term j and row r (oracle.cref.cosine_matrix; 0.0 for a
    acc = p_0, arg = 0              zero norm)
    for j = 1 .. J-1:  if p_j > acc (max) / p_j < acc (min):  acc = p_j, arg = j
    F(c, r) = acc,  T(c, r) = arg

The compare is strict: the first term wins a tie and +0.0 is never replaced by -0.0.  Rows are ranked by (F DESCENDING,
row id ascending) for both ops over the live rows the query's mask selects, ``F > min_score`` is a strict filter on the raw
value, the first k are kept, -1 / 0.0 padded (T: -1).  The score is stated twice over the same cosine matrix:

  (A) ``fold_scores_loop``   a Python-float loop per row, exactly the lines above;
  (B) ``fold_scores``        array-wise with an explicit loop over j and ``np.where`` on the strict compare (never np.max /
                             np.argmax: their choice among tied zeros of either sign is another function).

Both are ranked by tests/mask_ref.py ``masked_topk_from_scores``.  tests/test_fold_cpu.py holds them against each other;
the GPU tests compare with (A).  Also here: the cases, weight sets and the flag-0 condition of the scan test
(tests/test_fold_gpu.py), which the CPU file needs to prove the scan test's precondition without a GPU, and the model of
the reference's two-step linking (src/components/pre_llm_injector.py:238-249) that ``similarity.linked_similarities`` is
held against.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import cref
from tests import mask_ref as MR
from tests.scored_ref import CS, DTS, JS, KS, NQ, W_MAX, W_MIN, rank_pair, scan_selections, slack_m, term_rows  # noqa: F401

OPS = ("max", "min")
WEIGHT_SETS = ("ones", "signed", "wide")


def weights_of(name: str, J: int):
    """The scan test's weight sets, as Python floats."""
    if name == "ones":
        return [1.0] * J
    if name == "signed":
        return [(1.0, 1.0, -0.5)[j % 3] for j in range(J)]
    if name == "wide":
        return [(-1.0) ** j * 2.0 ** ((j % 5) - 2) for j in range(J)]
    raise KeyError(name)


FOLD_C = 2.0 ** -21                 # the bound's constant beside cert_eps (two roundings of 2^-24, slack)


def eps_fold(D: int, A: float) -> float:
    """The bound of the scanned score against F inside the domain: A (cert_eps(D) + 2^-21), A = max |w_j|."""
    return A * (MR.cert_eps(D) + FOLD_C)


def abs_max(w) -> float:
    a = 0.0
    for x in w:
        if abs(float(x)) > a:
            a = abs(float(x))
    return a


def fold_scores_loop(e, w, op):
    """(A).  e [J, n] fp64 cosines, w [J], op -> (F [n] fp64, T [n] int32)."""
    assert op in OPS
    e = np.asarray(e, dtype=np.float64)
    J, n = e.shape
    F = np.empty(n, dtype=np.float64)
    T = np.empty(n, dtype=np.int32)
    for r in range(n):
        acc, arg = float(w[0]) * float(e[0, r]), 0
        for j in range(1, J):
            p = float(w[j]) * float(e[j, r])
            if (p > acc) if op == "max" else (p < acc):
                acc, arg = p, j
        F[r], T[r] = acc, arg
    return F, T


def fold_scores(e, w, op):
    """(B)."""
    assert op in OPS
    e = np.asarray(e, dtype=np.float64)
    acc = np.float64(w[0]) * e[0]
    arg = np.zeros(e.shape[1], dtype=np.int32)
    for j in range(1, e.shape[0]):
        p = np.float64(w[j]) * e[j]
        take = (p > acc) if op == "max" else (p < acc)
        acc = np.where(take, p, acc)
        arg = np.where(take, np.int32(j), arg).astype(np.int32)
    return acc, arg


def terms_of_rows(T, out_rows, base=0):
    """T [C, n] and the ranked rows [C, k] -> T of each returned row, -1 where the row is -1."""
    out = np.full(out_rows.shape, -1, dtype=np.int32)
    for c in range(out_rows.shape[0]):
        hit = out_rows[c] >= 0
        out[c, hit] = T[c][out_rows[c, hit] - base]
    return out


def fold_topk(terms, weights, rows, sel, k, op, dtype="f16", min_score=None, base=0, scores=fold_scores_loop):
    """terms [C,J,D] and rows [n,D] (uint16 bit patterns, rows in row-id order), weights [C][J], sel bool [C,n] or None
    -> (rows [C,k] int64, scores [C,k] fp64, terms [C,k] int32) by statement (A) (``scores=fold_scores`` for (B))."""
    terms = np.ascontiguousarray(terms)
    C, J, D = terms.shape
    n = rows.shape[0]
    if sel is None:
        sel = np.ones((C, n), dtype=bool)
    F = np.zeros((C, n), dtype=np.float64)
    T = np.zeros((C, n), dtype=np.int32)
    if n:
        e = cref.cosine_matrix(terms.reshape(C * J, D), np.ascontiguousarray(rows), dtype=dtype).reshape(C, J, n)
        for c in range(C):
            F[c], T[c] = scores(e[c], weights[c], op)
    r, s = MR.masked_topk_from_scores(F, sel, k, min_score=min_score, base=base)
    return r, s, terms_of_rows(T, r, base)


# ---- the scan test's cases --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scan_scores(D, dtype, shape, J, wname, op):
    """(F, T) [3, live rows] of the three fold queries of (J, weight set, op) on the tile-scan dataset, by (A), from the
    shared oracle matrix; the weights [J]."""
    _, _, _, live = MR.host_dataset(D, dtype, shape)
    w = weights_of(wname, J)
    ft = [fold_scores_loop(live[term_rows(c, J)], w, op) for c in range(max(CS))]
    return np.stack([f for f, _ in ft]), np.stack([t for _, t in ft]), w


def flag0_ok(best_first, k: int, D: int, A: float) -> bool:
    """best_first: one query's exact selected F, descending.  True when rank k and rank M + 1 are more than
    4 x eps_fold(D, A) apart, or when there is no rank M + 1 (everything is re-scored exactly): the fast path must then
    certify the query."""
    pair = rank_pair(best_first, k)
    return pair is None or bool(pair[0] - pair[1] > 4 * eps_fold(D, A))


def margin(best_first, k: int, D: int, A: float) -> float:
    """(rank k - rank M + 1) / eps_fold, inf when there is no rank M + 1."""
    pair = rank_pair(best_first, k)
    return np.inf if pair is None else float((pair[0] - pair[1]) / eps_fold(D, A))


# ---- the reference's two-step linking -----------------------------------------------------------------------------------
def reference_merge(batch_similarities, top_k_similar_batch):
    """src/components/pre_llm_injector.py:238-249 restated: the maximum score per chunk id over the batch's result lists
    (a dict, so first-seen order), a stable descending sort, the first ``top_k_similar_batch``."""
    final_scores = {}
    for chunk_similarities in batch_similarities:
        for chunk_id, score in chunk_similarities:
            if chunk_id not in final_scores or score > final_scores[chunk_id]:
                final_scores[chunk_id] = score
    final_score_list = sorted(final_scores.items(), key=lambda x: x[1], reverse=True)
    return final_score_list[:top_k_similar_batch]


def reference_linking(cos, ids, top_k_each, top_k_final, sel=None):
    """The two steps on a cosine matrix: cos [Q, n] fp64 (row q = ``None`` for a failed embedding, which contributes
    ``[]``), ids [n], sel bool [n] or None.  Each embedding's top ``top_k_each`` by (score desc, row asc), then
    ``reference_merge``."""
    lists = []
    for row in cos:
        if row is None:
            lists.append([])
            continue
        keep = np.ones(len(ids), dtype=bool) if sel is None else np.asarray(sel, dtype=bool)
        r, s = MR.masked_topk_from_scores(np.asarray(row)[None], keep[None], top_k_each)
        lists.append([(ids[i], float(v)) for i, v in zip(r[0], s[0]) if i >= 0])
    return reference_merge(lists, top_k_final)


def fold_linking(cos, ids, top_k_final, sel=None, group=16):
    """What ``similarity.linked_similarities`` computes on the fold route, on the same matrix: the usable embeddings in
    groups of at most ``group`` (the last one filled with copies of its first), each group's top ``top_k_final`` by the
    max fold with unit weights, the lists max-merged per row, (score desc, row asc), the first ``top_k_final``."""
    ok = [np.asarray(row, dtype=np.float64) for row in cos if row is not None]
    J = min(len(ok), group)
    C = -(-len(ok) // J)
    ok += [ok[(C - 1) * J]] * (C * J - len(ok))
    keep = np.ones(len(ids), dtype=bool) if sel is None else np.asarray(sel, dtype=bool)
    best = {}
    for c in range(C):
        F, _ = fold_scores_loop(np.stack(ok[c * J:(c + 1) * J]), [1.0] * J, "max")
        r, s = MR.masked_topk_from_scores(F[None], keep[None], top_k_final)
        for i, v in zip(r[0], s[0]):
            if i >= 0 and (i not in best or v > best[i]):
                best[int(i)] = float(v)
    top = sorted(best.items(), key=lambda x: (-x[1], x[0]))[:top_k_final]
    return [(ids[i], v) for i, v in top]


# ---- the certificate's A ---------------------------------------------------------------------------------------------------

def certificate_gap_case(D=128, n=16, delta=0.0161):
    """-> (rows uint16 [n, D] fp16 bits, term uint16 [D], gap): row 0 is the term itself (cosine 1.0), every other row
    leans away from it by ``delta`` in a coordinate of its own, so rank 1 and every later rank are ``gap`` ~ delta^2 / 2
    apart: between 4 eps_fold(D, 1) and eps_fold(D, 16) - eps_fold(D, 1)."""
    rows = np.zeros((n, D), dtype=np.float16)
    rows[:, 0] = 1.0
    for i in range(1, n):
        rows[i, i] = delta
    bits = np.ascontiguousarray(rows).view(np.uint16)
    cos = cref.cosine_matrix(bits[:1], bits, dtype="f16")[0]
    assert cos[0] == 1.0 and len(set(cos[1:].tolist())) == 1
    return bits, bits[0], float(cos[0] - cos[1])
