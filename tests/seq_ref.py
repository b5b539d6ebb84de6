"""Test oracle of the sequence search (include/vidmem.h vm_topk_cosine_seq).

Contract: row r is ELIGIBLE for a sequence iff it is live and the sequence's mask selects it.  A CHAIN is rows
r_0 < ... < r_{J-1}, all eligible, 1 <= r_j - r_{j-1} <= G, no row in r_{j-1}+1 .. r_j with a tag break against its
predecessor (tests/clip_ref.tag_breaks).  P_0(r) = 0.0 + e_0(r); P_j(r) = (the largest P_{j-1}(r - d) over the allowed d in
1 .. G, ties to the smallest d) + e_j(r); A(r) = P_{J-1}(r) / J; r is an END iff A(r) exists.  r is a PEAK iff it ranks
before every END r' != r with |r' - r| < min_sep in (A desc, end row asc); the result is the peaks ranked the same way, the
score_mode mapping, the strict ``> min_score`` filter, first k, with the chain followed back from the end and its step
scores; 0.0 / -1 / -1 / 0.0 padded.  Three statements over oracle.cref.cosine_matrix' bit-exact raw cosines:

  (A) ``seq_topk``        vectorised layers: one array expression per (layer, d);
  (B) ``seq_topk_loop``   a plain Python loop per row and d, with the back-trace;
  (C) ``seq_brute``       every chain enumerated (tiny inputs): A(r) = the maximum over the chains ending at r of the
                          left-to-right rounded sum, / J - the consequence of monotone rounding the contract states.

tests/test_seq_cpu.py holds them against each other; the GPU tests compare with (A).  Also here: ``eps_seq``, the bound of
the fp32 stage, ``margin``, the reference's own distance from the certificate's condition (the clip oracle's, restated for
END rows), SEQ_SEG, the end rows per block of the align kernel (csrc/topk_seq.hip), and the planted sequences of the GPU
tests.
"""
from __future__ import annotations

import itertools

import numpy as np

from tests import clip_ref as CL
from tests.domain_ref import cert_eps
from tests.support import to_bits

SEQ_SEG = 768          # csrc/topk_seq.hip: end rows per block of the align kernel
NEG = -np.inf


def eps_seq(D: int, J: int) -> float:
    """|Bf(r) - A(r)| <= eps_seq inside the certificate's domain.  e~_j = (double)S / ||q_j|| lies within
    cert_eps(D) of e_j.  The layers are kept in fp64: a maximum moves no more than its most-moved argument, so P~_j lies
    within (j + 1) cert_eps(D) + (j + 1) 2^-52 * 16 of P_j, and A~ = P~_{J-1} / J within cert_eps(D) + 2^-47.  The one fp32
    rounding of |A~| <= 1 + eps adds less than 2^-24 * 1.001.  Together below cert_eps(D) + 2^-23 for every J <= 16: the
    clip search's eps_w, whose peak filter and certificate the sequence search runs unchanged."""
    assert 1 <= J <= 16
    return cert_eps(D) + 2.0 ** -23


def eligible(n, C, sel=None) -> np.ndarray:
    if sel is None:
        return np.ones((C, n), bool)
    sel = np.asarray(sel, dtype=bool)
    assert sel.shape == (C, n), sel.shape
    return sel


# ---- (A) ---------------------------------------------------------------------------------------------------------
def layers(S, elig, brk, G):
    """S [J, n] raw cosines, elig / brk bool [n] -> (P_{J-1} [n] with -inf where it does not exist, pred [J, n] = the d each
    cell took, 0 = none)."""
    J, n = S.shape
    P = np.where(elig, 0.0 + S[0], NEG)
    pred = np.zeros((J, n), np.int64)
    for j in range(1, J):
        best = np.full(n, NEG)
        bd = np.zeros(n, np.int64)
        blocked = np.zeros(n, bool)
        for d in range(1, min(G, n - 1) + 1):
            blocked[d - 1:] |= brk[:n - d + 1]              # a break on row r - (d - 1): in (r - d, r]
            cand = np.full(n, NEG)
            cand[d:] = P[:-d]
            cand[blocked] = NEG
            better = cand > best                            # strict: ties stay with the smaller d
            best = np.where(better, cand, best)
            bd = np.where(better, d, bd)
        exists = elig & (best > NEG)
        with np.errstate(invalid="ignore"):
            P = np.where(exists, best + S[j], NEG)
        pred[j] = np.where(exists, bd, 0)
    return P, pred


def end_scores(S, elig, brk, G):
    """-> (A [n], is_end bool [n], pred [J, n])."""
    P, pred = layers(S, elig, brk, G)
    ends = P > NEG
    return np.where(ends, P / float(S.shape[0]), NEG), ends, pred


def trace(pred, S, r):
    J = S.shape[0]
    rows, scores = np.zeros(J, np.int64), np.zeros(J, np.float64)
    for j in range(J - 1, -1, -1):
        rows[j], scores[j] = r, S[j, r]
        r -= int(pred[j, r])
    return rows, scores


def from_scores(S, elig, brk, k, G, min_sep, score_mode=0, min_score=None, base=0):
    """One sequence from its raw step scores S [J, n] -> (rows [k], scores [k], step_rows [k, J], step_scores [k, J])."""
    J = S.shape[0]
    A, ends, pred = end_scores(S, elig, brk, G)
    out_r, out_s = CL.rank(A, CL.peak_mask(A, ends, min_sep), k, score_mode, min_score, base)
    out_sr = np.full((k, J), -1, np.int64)
    out_ss = np.zeros((k, J), np.float64)
    for i in range(k):
        if out_r[i] >= 0:
            tr, ts = trace(pred, S, int(out_r[i]) - base)
            out_sr[i], out_ss[i] = tr + base, ts
    return out_r, out_s, out_sr, out_ss


def seq_topk(steps, rows, k, G, min_sep, dtype="f16", tags=None, sel=None, max_gap_ms=-1, score_mode=0, min_score=None,
             base=0):
    """(A).  steps [C, J, D], rows [n, D] (uint16 bit patterns, row-id order), tags [n] or None, sel bool [C, n] or None ->
    (rows [C,k] int64 END row ids = base + index, scores [C,k] fp64, step_rows [C,k,J] int64, step_scores [C,k,J] fp64)."""
    steps = np.ascontiguousarray(steps)
    C, J = steps.shape[0], steps.shape[1]
    n = rows.shape[0]
    el = eligible(n, C, sel)
    brk = np.zeros(n, bool) if tags is None else CL.tag_breaks(tags, max_gap_ms)
    out = (np.full((C, k), -1, np.int64), np.zeros((C, k), np.float64), np.full((C, k, J), -1, np.int64),
           np.zeros((C, k, J), np.float64))
    for c in range(C):
        if n == 0:
            continue
        got = from_scores(CL.frame_scores(steps[c], rows, dtype), el[c], brk, k, G, min_sep, score_mode, min_score, base)
        for o, g in zip(out, got):
            o[c] = g
    return out


# ---- (B) ---------------------------------------------------------------------------------------------------------
def seq_topk_loop(steps, rows, k, G, min_sep, dtype="f16", tags=None, sel=None, max_gap_ms=-1, score_mode=0,
                  min_score=None, base=0):
    """(B)."""
    steps = np.ascontiguousarray(steps)
    C, J = steps.shape[0], steps.shape[1]
    n = rows.shape[0]
    tg = None if tags is None else [int(t) for t in tags]
    out_r = np.full((C, k), -1, np.int64)
    out_s = np.zeros((C, k), np.float64)
    out_sr = np.full((C, k, J), -1, np.int64)
    out_ss = np.zeros((C, k, J), np.float64)
    for c in range(C):
        S = CL.frame_scores(steps[c], rows, dtype)
        ok = [True] * n if sel is None else [bool(x) for x in sel[c]]
        P = [dict() for _ in range(J)]
        pred = [dict() for _ in range(J)]
        for r in range(n):
            if ok[r]:
                P[0][r] = 0.0 + float(S[0, r])
        for j in range(1, J):
            for r in range(n):
                if not ok[r]:
                    continue
                best, bd = None, 0
                for d in range(1, G + 1):
                    if r - d < 0:
                        break
                    if tg is not None and CL._breaks(tg[r - d], tg[r - d + 1], max_gap_ms):
                        break                               # every longer step crosses this break too
                    if (r - d) in P[j - 1] and (best is None or P[j - 1][r - d] > best):
                        best, bd = P[j - 1][r - d], d
                if best is not None:
                    P[j][r] = best + float(S[j, r])
                    pred[j][r] = r - bd
        A = {r: v / float(J) for r, v in P[J - 1].items()}
        peaks = []
        for r in A:
            is_peak = True
            for r2 in range(r - min_sep + 1, r + min_sep):
                if r2 == r or r2 not in A:
                    continue
                if A[r2] > A[r] or (A[r2] == A[r] and r2 < r):
                    is_peak = False
            if is_peak:
                peaks.append(r)
        peaks.sort(key=lambda r: (-A[r], r))
        i = 0
        for r in peaks:
            shown = (1.0 + A[r]) / 2.0 if score_mode == 1 else A[r]
            if min_score is not None and not shown > min_score:
                continue
            if i == k:
                break
            out_r[c, i], out_s[c, i] = base + r, shown
            at = r
            for j in range(J - 1, -1, -1):
                out_sr[c, i, j], out_ss[c, i, j] = base + at, S[j, at]
                at = pred[j].get(at, at)
            i += 1
    return out_r, out_s, out_sr, out_ss


# ---- (C) ---------------------------------------------------------------------------------------------------------
def seq_brute(step_scores, elig, brk, G):
    """S [J, n] -> {end row: A}: every chain enumerated, its sum taken from 0.0 left to right, the maximum per end row
    divided by J once."""
    J, n = step_scores.shape
    best = {}
    for chain in itertools.combinations(range(n), J):
        if not all(elig[r] for r in chain):
            continue
        good = True
        for a, b in zip(chain, chain[1:]):
            if b - a > G or brk[a + 1:b + 1].any():
                good = False
        if not good:
            continue
        s = 0.0
        for j, r in enumerate(chain):
            s = s + float(step_scores[j, r])
        if chain[-1] not in best or s > best[chain[-1]]:
            best[chain[-1]] = s
    return {r: s / float(J) for r, s in best.items()}


# ---- the reference's own distance from the certificate's condition -------------------------------------------------
def margin(steps, rows, k, G, min_sep, dtype="f16", tags=None, sel=None, max_gap_ms=-1):
    """tests/clip_ref.margin restated for END rows -> (smallest margin in units of eps_seq(D, J) over the sequences, whether
    the best M end rows that could be possible peaks always held k exact peaks).  An end row can be a POSSIBLE peak of the
    fp32 stage only if no competitor's A exceeds its own by more than 4 eps_seq; the margin is (A of the k-th exact peak - A
    of the (M+1)-th best such end row) / eps_seq.  The certificate needs more than 2.  inf when there are at most M."""
    steps = np.ascontiguousarray(steps)
    C, J, D = steps.shape
    n = rows.shape[0]
    M = k + max(k // 4, 8)
    e = eps_seq(D, J)
    el = eligible(n, C, sel)
    brk = np.zeros(n, bool) if tags is None else CL.tag_breaks(tags, max_gap_ms)
    worst, held = np.inf, True
    for c in range(C):
        A, ok, _ = end_scores(CL.frame_scores(steps[c], rows, dtype), el[c], brk, G)
        far = np.zeros(n, bool)
        with np.errstate(invalid="ignore"):
            for d in range(1, min(min_sep, n)):
                far[d:] |= ok[:-d] & (A[:-d] > A[d:] + 4 * e)
                far[:-d] |= ok[d:] & (A[d:] > A[:-d] + 4 * e)
        possible = np.nonzero(ok & ~far)[0]
        if possible.size <= M:
            continue
        order = possible[np.lexsort((possible, -A[possible]))]
        peaks = CL.peak_mask(A, ok, min_sep)
        top = order[:M]
        exact = top[peaks[top]]
        if exact.size < k:
            held = False
            continue
        worst = min(worst, (A[exact[k - 1]] - A[order[M]]) / e)
    return worst, held


# ---- test data: planted sequences ------------------------------------------------------------------------------------
def chains_from(starts, J, G, seed):
    """int64 [C, J]: from each start, J rows at cumulative random gaps in 1 .. G."""
    rng = np.random.default_rng(seed)
    gaps = rng.integers(1, G + 1, (len(starts), J))
    gaps[:, 0] = 0
    return np.asarray(starts, np.int64)[:, None] + np.cumsum(gaps, axis=1)


def steps_at(bits, dtype, chains, seed, noise=0.1) -> np.ndarray:
    """uint16 bits [C, J, D]: the stored rows of each chain plus ``noise`` x unit noise."""
    rng = np.random.default_rng(seed)
    vals = CL.from_bits(bits, dtype)
    out = vals[np.asarray(chains)].astype(np.float32)
    out = out + noise * CL._unit(rng.standard_normal(out.shape))
    return to_bits(out, dtype)


def steps_from(bits, dtype, starts, J, G, seed, noise=0.1):
    """-> (steps uint16 [C, J, D], chains int64 [C, J]): a sequence = J stored rows at cumulative random gaps in 1 .. G from
    each start, plus ``noise`` x unit noise."""
    chains = chains_from(starts, J, G, seed)
    return steps_at(bits, dtype, chains, seed + 1, noise), chains


def pick_starts(n, J, G, C, seed):
    return [int(s) for s in np.random.default_rng(seed).integers(0, n - (J - 1) * G, C)]
