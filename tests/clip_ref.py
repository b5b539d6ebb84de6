"""Test oracle of the clip search (include/vidmem.h vm_topk_cosine_clip).

Contract: window r = live rows r .. r+L-1; VALID iff all L rows are live and no row r+1 .. r+L-1 has a tag break against
its predecessor (the tag part of tests/events_ref.opens); IN SCOPE iff every row's tag lies in the clip's [lo, hi];
W(r) = (e_0 + ... + e_{L-1}) / L over the raw reference cosines e_i = cos(clip frame i, row r+i), summed from 0.0 left to
right; r is a PEAK iff it ranks before every valid in-scope window r' != r with |r' - r| < min_sep in (W desc, start asc);
the result is the peaks ranked the same way, the score_mode mapping, the strict ``> min_score`` filter, first k; -1 / 0.0
padded.  Two independent statements over oracle.cref.cosine_matrix' bit-exact raw cosines:

  (A) ``clip_topk``       vectorised: acc = acc + S[i, i:i+nw] for i = 0 .. L-1, then / L; validity, scope and peak masks
                          as array expressions; lexsort;
  (B) ``clip_topk_loop``  a plain Python loop per window and per competitor.

tests/test_clip_cpu.py holds them against each other; the GPU tests compare with (A).  Also here: the scene-structured
test "video" of the GPU tests and ``margin``, the reference's own distance from the certificate's condition.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import cref
from tests.domain_ref import cert_eps
from tests.support import to_bits  # noqa: F401  (CL.to_bits for the other refs)

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
MS_BITS = 40
MS_MASK = (1 << MS_BITS) - 1


def eps_w(D: int) -> float:
    """cert_eps(D) + 2^-23 (csrc/topk_clip.hip clip_eps_w)."""
    return cert_eps(D) + 2.0 ** -23


def scope_arrays(scopes, C):
    if scopes is None:
        return None, None
    sc = np.asarray(scopes, dtype=np.int64)
    if sc.ndim == 1:
        sc = np.tile(sc, (C, 1))
    assert sc.shape == (C, 2), sc.shape
    return sc[:, 0].copy(), sc[:, 1].copy()


def frame_scores(clip, rows, dtype):
    """[L, n] raw reference cosines of the clip's frames against every row."""
    n = rows.shape[0]
    if n == 0:
        return np.zeros((clip.shape[0], 0), np.float64)
    return cref.cosine_matrix(np.ascontiguousarray(clip), np.ascontiguousarray(rows), dtype=dtype)


# ---- (A) ---------------------------------------------------------------------------------------------------------
def tag_breaks(tags, max_gap_ms=-1) -> np.ndarray:
    """bool [n]: row i has a tag break against row i - 1 (False for row 0)."""
    tags = np.asarray(tags, dtype=np.int64)
    out = np.zeros(tags.size, bool)
    if tags.size < 2:
        return out
    tp, tc = tags[:-1], tags[1:]
    up, uc = tp == INT64_MIN, tc == INT64_MIN
    step = (tc & MS_MASK) - (tp & MS_MASK)
    timed = ~up & ~uc
    brk = up != uc
    brk |= timed & ((tp >> MS_BITS) != (tc >> MS_BITS))
    if max_gap_ms >= 0:
        brk |= timed & ((step < 0) | (step > max_gap_ms))
    out[1:] = brk
    return out


def window_mask(n, L, tags=None, lo=None, hi=None, max_gap_ms=-1) -> np.ndarray:
    """bool [nw], nw = max(n - L + 1, 0): window r is valid and in scope."""
    nw = max(n - L + 1, 0)
    ok = np.ones(nw, bool)
    if tags is None or nw == 0:
        return ok
    tags = np.asarray(tags, dtype=np.int64)
    brk = tag_breaks(tags, max_gap_ms)
    for i in range(1, L):
        ok &= ~brk[i:i + nw]
    if lo is not None:
        ins = (tags >= lo) & (tags <= hi)
        for i in range(L):
            ok &= ins[i:i + nw]
    return ok


def window_scores(S, L) -> np.ndarray:
    """S [L, n] -> W [nw]: the sum from 0.0 left to right, then one division."""
    n = S.shape[1]
    nw = max(n - L + 1, 0)
    acc = np.zeros(nw, np.float64)
    for i in range(L):
        acc = acc + S[i, i:i + nw]
    return acc / L


def peak_mask(W, ok, min_sep) -> np.ndarray:
    nw = W.size
    beaten = np.zeros(nw, bool)
    for d in range(1, min_sep):
        if d >= nw:
            break
        # the competitor d rows EARLIER ranks before r when its W is >= W(r); the one d rows LATER when it is > W(r)
        beaten[d:] |= ok[:-d] & (W[:-d] >= W[d:])
        beaten[:-d] |= ok[d:] & (W[d:] > W[:-d])
    return ok & ~beaten


def rank(W, cand_mask, k, score_mode=0, min_score=None, base=0):
    shown = (1.0 + W) / 2.0 if score_mode == 1 else W
    cand = np.nonzero(cand_mask)[0]
    order = cand[np.lexsort((cand, -W[cand]))]
    if min_score is not None:
        order = order[shown[order] > min_score]
    best = order[:k]
    out_r = np.full(k, -1, np.int64)
    out_s = np.zeros(k, np.float64)
    out_r[:best.size] = base + best
    out_s[:best.size] = shown[best]
    return out_r, out_s


def clip_topk(clips, rows, k, min_sep, dtype="f16", tags=None, scopes=None, max_gap_ms=-1, score_mode=0, min_score=None,
              base=0):
    """(A).  clips [C, L, D], rows [n, D] (uint16 bit patterns, row-id order), tags [n] or None -> (rows [C,k] int64 start
    row ids = base + index, scores [C,k] fp64)."""
    clips = np.ascontiguousarray(clips)
    C, L = clips.shape[0], clips.shape[1]
    n = rows.shape[0]
    lo, hi = scope_arrays(scopes, C)
    out_r = np.full((C, k), -1, np.int64)
    out_s = np.zeros((C, k), np.float64)
    for c in range(C):
        if n < L:
            continue
        W = window_scores(frame_scores(clips[c], rows, dtype), L)
        ok = window_mask(n, L, tags, None if lo is None else lo[c], None if hi is None else hi[c], max_gap_ms)
        out_r[c], out_s[c] = rank(W, peak_mask(W, ok, min_sep), k, score_mode, min_score, base)
    return out_r, out_s


# ---- (B) ---------------------------------------------------------------------------------------------------------
def _breaks(tp, tc, max_gap_ms) -> bool:
    up, uc = tp == INT64_MIN, tc == INT64_MIN
    if up != uc:
        return True
    if up:
        return False
    if (tp >> MS_BITS) != (tc >> MS_BITS):
        return True
    step = (tc & MS_MASK) - (tp & MS_MASK)
    return max_gap_ms >= 0 and (step < 0 or step > max_gap_ms)


def clip_topk_loop(clips, rows, k, min_sep, dtype="f16", tags=None, scopes=None, max_gap_ms=-1, score_mode=0,
                   min_score=None, base=0):
    """(B)."""
    clips = np.ascontiguousarray(clips)
    C, L = clips.shape[0], clips.shape[1]
    n = rows.shape[0]
    lo, hi = scope_arrays(scopes, C)
    tg = None if tags is None else [int(t) for t in tags]
    out_r = np.full((C, k), -1, np.int64)
    out_s = np.zeros((C, k), np.float64)
    for c in range(C):
        S = frame_scores(clips[c], rows, dtype)
        W, ok = {}, {}
        for r in range(n):
            good = r + L <= n
            if good and tg is not None:
                for i in range(L):
                    if i > 0 and _breaks(tg[r + i - 1], tg[r + i], max_gap_ms):
                        good = False
                    if lo is not None and not (int(lo[c]) <= tg[r + i] <= int(hi[c])):
                        good = False
            ok[r] = good
            if good:
                s = 0.0
                for i in range(L):
                    s = s + float(S[i, r + i])
                W[r] = s / float(L)
        peaks = []
        for r in range(n):
            if not ok[r]:
                continue
            is_peak = True
            for r2 in range(r - min_sep + 1, r + min_sep):
                if r2 == r or r2 < 0 or r2 >= n or not ok[r2]:
                    continue
                if W[r2] > W[r] or (W[r2] == W[r] and r2 < r):
                    is_peak = False
            if is_peak:
                peaks.append(r)
        peaks.sort(key=lambda r: (-W[r], r))
        j = 0
        for r in peaks:
            shown = (1.0 + W[r]) / 2.0 if score_mode == 1 else W[r]
            if min_score is not None and not shown > min_score:
                continue
            if j == k:
                break
            out_r[c, j], out_s[c, j] = base + r, shown
            j += 1
    return out_r, out_s


# ---- the reference's own distance from the certificate's condition -------------------------------------------------
def margin(clips, rows, k, min_sep, dtype="f16", tags=None, scopes=None, max_gap_ms=-1):
    """-> (smallest margin in units of eps_w(D) over the clips, whether the best M windows that could be possible peaks
    always held k exact peaks).  Per clip: a window can be a POSSIBLE peak of the fp32 stage only if no competitor's W
    exceeds its own by more than 4 eps_w (each fp32 window score lies within eps_w of W and the stage allows 2 eps_w); the
    margin is (W of the k-th exact peak - W of the (M+1)-th best such window) / eps_w.  The certificate needs the
    difference of the fp32 image of the latter to be above eps_w: more than 2 here.  inf when there are at most M."""
    clips = np.ascontiguousarray(clips)
    C, L, D = clips.shape
    n = rows.shape[0]
    M = k + max(k // 4, 8)
    e = eps_w(D)
    lo, hi = scope_arrays(scopes, C)
    worst, held = np.inf, True
    for c in range(C):
        W = window_scores(frame_scores(clips[c], rows, dtype), L)
        ok = window_mask(n, L, tags, None if lo is None else lo[c], None if hi is None else hi[c], max_gap_ms)
        nw = W.size
        far = np.zeros(nw, bool)
        for d in range(1, min(min_sep, nw)):
            far[d:] |= ok[:-d] & (W[:-d] > W[d:] + 4 * e)
            far[:-d] |= ok[d:] & (W[d:] > W[:-d] + 4 * e)
        possible = np.nonzero(ok & ~far)[0]
        if possible.size <= M:
            continue
        order = possible[np.lexsort((possible, -W[possible]))]
        peaks = peak_mask(W, ok, min_sep)
        top = order[:M]
        exact = top[peaks[top]]
        if exact.size < k:
            held = False
            continue
        worst = min(worst, (W[exact[k - 1]] - W[order[M]]) / e)
    return worst, held


# ---- test data: a scene-structured "video" ---------------------------------------------------------------------------
def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


@functools.lru_cache(maxsize=None)
def scene_video(n, D, dtype, seed):
    """uint16 bits [n, D]: scenes of 24 - 40 rows, row = normalise(scene centre + 0.5 x unit noise).  Made on the CPU
    (the same bytes with and without a GPU), once per process, never modified."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, D), np.float32)
    r = 0
    while r < n:
        size = min(int(rng.integers(24, 41)), n - r)
        centre = _unit(rng.standard_normal(D))
        out[r:r + size] = _unit(centre + 0.5 * _unit(rng.standard_normal((size, D))))
        r += size
    bits = to_bits(out, dtype)
    bits.setflags(write=False)
    return bits


def from_bits(bits, dtype) -> np.ndarray:
    import torch
    t = torch.from_numpy(np.array(bits).view(np.int16)).view(torch.float16 if dtype == "f16" else torch.bfloat16)
    return t.float().numpy()


def clips_from(bits, dtype, starts, L, seed, noise=0.1) -> np.ndarray:
    """uint16 bits [C, L, D]: L consecutive stored rows from each start plus ``noise`` x unit noise."""
    rng = np.random.default_rng(seed)
    vals = from_bits(bits, dtype)
    out = np.stack([vals[s:s + L] for s in starts]).astype(np.float32)
    out = out + noise * _unit(rng.standard_normal(out.shape))
    return to_bits(out, dtype)


def pick_starts(n, L, C, seed):
    return [int(s) for s in np.random.default_rng(seed).integers(0, n - L + 1, C)]
