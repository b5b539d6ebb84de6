"""Host-side model of ``vm_preprocess`` for tests/test_preprocess_cpu.py and tests/test_preprocess_gpu.py.

The definition of the operation is the expression in include/vidmem.h, which ``oracle.frames_ref.preprocess_ref`` states
in vectorised numpy.  This module holds

* ``CASES``         the one case table both tests run: every kernel instance ({f16, bf16} x {<16,768>, <14,640>, <0,0>}),
                    both layouts, the identity fast path, the sizes next to it that must not take it, degenerate sources,
                    integer ratios, the grid-stride wrap, misaligned frame pointers;
* ``scalar_model``  the header's definition once more, one output at a time with ``np.float32`` scalars (independent of
                    the oracle's vectorised helpers; small cases only);
* ``exact_fp64``    the same taps in float64 with the bound on ``|oracle - exact|`` that the fp32 roundings allow;
* ``bits16``        fp32 -> the int16 bit pattern of the f16 / bf16 value (round to nearest even, subnormals kept);
* ``census``        what a case's oracle output holds of the values a cast or a clamp can get wrong;
* ``emulate``       the kernel's own index and tap arithmetic (chunk index -> frame, channel, pixel; taps; cast) in numpy,
                    equal to the oracle when sound, and able to carry each of the planted ``DEFECTS``.

All comparisons are on bit patterns.
"""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple

import numpy as np

from oracle import frames_ref as F

NORMS = {
    "vit": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),
    "clip": ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)),
}
Case = namedtuple("Case", "name dtype layout S patch k_pad H W B norm recipe offset")
WRAP = None  # B of a wrap case: the GPU test computes it from the device, the CPU tests use WRAP_B_CPU
WRAP_B_CPU = 3


def _case(name, dtype, layout, S, patch, k_pad, H, W, B, norm="vit", recipe="random", offset=0):
    if layout == "chw":
        patch, k_pad = 0, 0
    return Case(name, dtype, layout, S, patch, k_pad, H, W, B, norm, recipe, offset)


def _table():
    t = []
    vit = dict(dtype="f16", S=224, patch=16, k_pad=768, norm="vit")
    clip = dict(dtype="bf16", S=336, patch=14, k_pad=640, norm="clip")
    # the two product specs: identity, a 16:9 downscale, odd sizes with an odd frame stride, a 40 x upscale, 1080p
    for tag, sp in (("vit", vit), ("clip", clip)):
        for H, W, B in ((sp["S"], sp["S"], 2), (360, 640, 2), (97, 131, 2), (7, 5, 2), (1080, 1920, 1)):
            for layout in ("chw", "patches"):
                t.append(_case(f"{tag}-{H}x{W}-{layout}", sp["dtype"], layout, sp["S"], sp["patch"], sp["k_pad"], H, W, B,
                               sp["norm"]))
    # one 4K frame per dtype (one layout each)
    t.append(_case("vit-2160x3840-patches", "f16", "patches", 224, 16, 768, 2160, 3840, 1, "vit"))
    t.append(_case("clip-2160x3840-chw", "bf16", "chw", 336, 14, 640, 2160, 3840, 1, "clip"))
    # identity fast path (<16,768>, H == W == S): bf16 at 224, both types at 64 and 32
    t.append(_case("fast-bf16-224", "bf16", "patches", 224, 16, 768, 224, 224, 2, "clip"))
    for dt in ("f16", "bf16"):
        for S in (32, 64):
            t.append(_case(f"fast-{dt}-{S}", dt, "patches", S, 16, 768, S, S, 3, "vit" if dt == "f16" else "clip"))
    # the other instance of each compile-time pair, away from the product type
    t.append(_case("p16-bf16-40x56", "bf16", "patches", 64, 16, 768, 40, 56, 2, "clip"))
    t.append(_case("p14-f16-97x131", "f16", "patches", 56, 14, 640, 97, 131, 2, "vit"))
    # generic patches (<0,0>): run-time divisors, pad regions of 0, 4 and 0 columns
    for dt, norm in (("f16", "vit"), ("bf16", "clip")):
        t.append(_case(f"generic-p8-k192-{dt}", dt, "patches", 64, 8, 192, 40, 56, 2, norm))
        t.append(_case(f"generic-p14-k592-{dt}", dt, "patches", 56, 14, 592, 97, 131, 2, norm))
        t.append(_case(f"generic-p32-k3072-{dt}", dt, "patches", 64, 32, 3072, 75, 50, 2, norm))
    t.append(_case("generic-p16-k776-f16", "f16", "patches", 32, 16, 776, 32, 32, 2, "vit"))  # identity size, not <16,768>
    t.append(_case("generic-p8-k256-bf16", "bf16", "patches", 32, 8, 256, 20, 28, 2, "vit"))  # 64 pad columns
    # one side equal to S: the fast path must not be taken
    for dt in ("f16", "bf16"):
        for H, W in ((64, 65), (63, 64), (64, 128)):
            t.append(_case(f"near-{dt}-{H}x{W}", dt, "patches", 64, 16, 768, H, W, 2, "vit" if dt == "f16" else "clip"))
    # sources in which both taps clamp to one pixel
    for H, W in ((1, 1), (1, 9), (9, 1)):
        t.append(_case(f"thin-f16-{H}x{W}-chw", "f16", "chw", 32, 0, 0, H, W, 3, "vit"))
        t.append(_case(f"thin-bf16-{H}x{W}-patches", "bf16", "patches", 32, 16, 768, H, W, 3, "clip"))
    # integer ratios: 2:1 both ways (every lam 0.5), 3:1 x 1:1 (every lam 0)
    for dt in ("f16", "bf16"):
        t.append(_case(f"ratio2-{dt}-random", dt, "chw", 32, 0, 0, 64, 64, 2, "vit" if dt == "f16" else "clip"))
        t.append(_case(f"ratio3x1-{dt}-random", dt, "patches", 32, 16, 768, 96, 32, 2, "vit" if dt == "f16" else "clip"))
    # frame recipes; rows of 127 / 128 under mean = std = 0.5 give exact +0.0 at 2:1 and values next to zero elsewhere
    for dt in ("f16", "bf16"):
        t.append(_case(f"rows127-{dt}-2to1", dt, "patches", 32, 16, 768, 64, 64, 2, "vit", "rows127"))
        t.append(_case(f"rows127-{dt}-97x131", dt, "chw", 64, 0, 0, 97, 131, 1, "vit", "rows127"))
        t.append(_case(f"rows127-{dt}-61x40", dt, "patches", 56, 14, 640, 61, 40, 1, "vit", "rows127"))
        t.append(_case(f"zeros-{dt}", dt, "patches", 32, 16, 768, 20, 28, 2, "vit" if dt == "f16" else "clip", "zeros"))
        t.append(_case(f"full-{dt}", dt, "chw", 32, 0, 0, 20, 28, 2, "vit" if dt == "f16" else "clip", "full"))
        t.append(_case(f"channels-{dt}", dt, "patches", 32, 8, 192, 20, 28, 2, "clip", "channels"))
        t.append(_case(f"corners-{dt}-up", dt, "chw", 32, 0, 0, 5, 7, 2, "vit" if dt == "f16" else "clip", "corners"))
        t.append(_case(f"corners-{dt}-down", dt, "patches", 32, 16, 768, 75, 50, 2, "clip", "corners"))
    # grid-stride wrap: more chunks than twice the threads of a capped grid, once per dtype, and once on the fast path
    t.append(_case("wrap-f16-40x56", "f16", "patches", 64, 16, 768, 40, 56, WRAP, "vit"))
    t.append(_case("wrap-bf16-40x56", "bf16", "patches", 64, 16, 768, 40, 56, WRAP, "clip"))
    t.append(_case("wrap-f16-identity", "f16", "patches", 64, 16, 768, 64, 64, WRAP, "vit"))
    # frames that start 1, 3 and 5 bytes into a larger buffer: identity sizes (byte loads, not the fast path) and one
    # general case
    for off in (1, 3, 5):
        t.append(_case(f"offset{off}-fast-f16-64", "f16", "patches", 64, 16, 768, 64, 64, 2, "vit", offset=off))
        t.append(_case(f"offset{off}-fast-bf16-32", "bf16", "patches", 32, 16, 768, 32, 32, 2, "clip", offset=off))
        t.append(_case(f"offset{off}-general-f16", "f16", "chw", 32, 0, 0, 97, 131, 2, "vit", offset=off))
    t.append(_case("offset3-fast-f16-224", "f16", "patches", 224, 16, 768, 224, 224, 1, "vit", offset=3))
    t.append(_case("offset8-fast-f16-64", "f16", "patches", 64, 16, 768, 64, 64, 2, "vit", offset=8))  # still aligned
    names = [c.name for c in t]
    assert len(set(names)) == len(names)
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}


def is_fast(case, aligned=None) -> bool:
    """Whether the kernel's identity fast path serves this case (csrc/context.hip)."""
    aligned = case.offset % 8 == 0 if aligned is None else aligned
    return (case.layout == "patches" and case.patch == 16 and case.k_pad == 768 and case.H == case.S
            and case.W == case.S and aligned)


def n_out(case, B=None) -> int:
    B = (case.B or WRAP_B_CPU) if B is None else B
    g = case.S // case.patch if case.layout == "patches" else 0
    return B * (g * g * case.k_pad if case.layout == "patches" else 3 * case.S * case.S)


def chunks_per_frame(case) -> int:
    return n_out(case, 1) // 8


def is_small(case) -> bool:
    """Cases the per-output Python loop of scalar_model runs on."""
    return case.S <= 32 and n_out(case) <= 3 * 32 * 32 * 3


def frames(case, B=None) -> np.ndarray:
    """uint8 [B, H, W, 3] BGR frames of a case, from a seed fixed by the case's name."""
    B = (case.B or WRAP_B_CPU) if B is None else B
    H, W = case.H, case.W
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    if case.recipe == "random":
        return rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    f = np.zeros((B, H, W, 3), np.uint8)
    if case.recipe == "zeros":
        pass
    elif case.recipe == "full":
        f[:] = 255
    elif case.recipe == "channels":
        f[..., 0], f[..., 1], f[..., 2] = 10, 128, 250
    elif case.recipe == "rows127":
        f[:] = (127 + (np.arange(H) & 1)).astype(np.uint8)[None, :, None, None]
    elif case.recipe == "corners":
        for b in range(B):
            for (y, x), v in (((0, 0), 255), ((0, W - 1), 200), ((H - 1, 0), 150), ((H - 1, W - 1), 100)):
                f[b, y, x] = (v, v - 20 - b, v - 40)
    else:
        raise ValueError(case.recipe)
    return f


def consts(case):
    """a = 1 / (255 std), b = -mean / std in fp32, as the host computes them."""
    mean, std = (np.asarray(v, np.float32) for v in NORMS[case.norm])
    a = (np.float32(1.0) / (np.float32(255.0) * std)).astype(np.float32)
    b = (-mean / std).astype(np.float32)
    return a, b


def oracle(case, fr=None) -> np.ndarray:
    """fp32 output of the oracle, flat in the output's memory order."""
    fr = frames(case) if fr is None else fr
    mean, std = NORMS[case.norm]
    return F.preprocess_ref(fr, case.S, mean, std, layout=case.layout, patch=case.patch, k_pad=case.k_pad).reshape(-1)


@functools.lru_cache(maxsize=None)
def oracle_cached(name):
    out = oracle(BY_NAME[name])
    out.setflags(write=False)
    return out


# ---- casts ---------------------------------------------------------------------------------------------------------
def _bf16_bits(x, mode="rne"):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    if mode == "rne":
        u = u + 0x7FFF + ((u >> 16) & 1)
    elif mode == "half_away":
        u = u + 0x8000
    elif mode != "rtz":
        raise ValueError(mode)
    return (u >> 16).astype(np.uint16).view(np.int16)


def _f16_bits(x, mode="rne"):
    x = np.ascontiguousarray(x, np.float32)
    r = x.astype(np.float16)  # IEEE round to nearest even, subnormals kept
    if mode == "rne":
        return r.view(np.int16)
    x64, r64 = x.astype(np.float64), r.astype(np.float64)
    if mode == "rtz":  # step back whatever was rounded away from zero
        back = np.nextafter(r, np.float16(0))
        return np.where(np.abs(r64) > np.abs(x64), back, r).view(np.int16)
    if mode == "half_away":  # a tie that went to the even neighbour nearer zero goes to the other one
        with np.errstate(over="ignore"):  # the neighbour of the largest f16 is inf
            away = np.nextafter(r, np.where(x64 < 0, -np.inf, np.inf).astype(np.float16))
        tie = (np.abs(x64 - r64) == np.abs(away.astype(np.float64) - x64)) & (x64 != r64)
        return np.where(tie & (np.abs(r64) < np.abs(x64)), away, r).view(np.int16)
    raise ValueError(mode)


def bits16(x, dtype, mode="rne") -> np.ndarray:
    """int16 view of fp32 ``x`` cast to f16 / bf16 (all values here are finite and far from overflow)."""
    return (_f16_bits if dtype == "f16" else _bf16_bits)(x, mode)


# ---- the definition, one output at a time -------------------------------------------------------------------------------
def _tap_scalar(d, n, S):
    f32 = np.float32
    scale = f32(n) / f32(S)
    src = f32(f32(scale * f32(f32(d) + f32(0.5))) - f32(0.5))
    if src < f32(0.0):
        src = f32(0.0)
    i0 = min(int(np.floor(src)), n - 1)
    i1 = min(i0 + 1, n - 1)
    return i0, i1, f32(src - f32(i0))


def scalar_model(case, fr=None) -> np.ndarray:
    """include/vidmem.h's expression per output element, np.float32 scalars, one rounding per operation; fp32, flat in
    the output's memory order."""
    fr = frames(case) if fr is None else fr
    f32 = np.float32
    B, H, W, _ = fr.shape
    S, p = case.S, case.patch
    a, b = consts(case)
    ys = [_tap_scalar(d, H, S) for d in range(S)]
    xs = [_tap_scalar(d, W, S) for d in range(S)]
    one = f32(1.0)
    chw = np.zeros((B, 3, S, S), np.float32)
    for bb in range(B):
        for c in range(3):
            ch = 2 - c
            for oy in range(S):
                y0, y1, ly = ys[oy]
                for ox in range(S):
                    x0, x1, lx = xs[ox]
                    p00, p01 = f32(fr[bb, y0, x0, ch]), f32(fr[bb, y0, x1, ch])
                    p10, p11 = f32(fr[bb, y1, x0, ch]), f32(fr[bb, y1, x1, ch])
                    top = f32(f32(f32(one - lx) * p00) + f32(lx * p01))
                    bot = f32(f32(f32(one - lx) * p10) + f32(lx * p11))
                    val = f32(f32(f32(one - ly) * top) + f32(ly * bot))
                    chw[bb, c, oy, ox] = f32(f32(val * a[c]) + b[c])
    if case.layout == "chw":
        return chw.reshape(-1)
    g = S // p
    out = np.zeros((B, g * g, case.k_pad), np.float32)
    for bb in range(B):
        for gy in range(g):
            for gx in range(g):
                for c in range(3):
                    for py in range(p):
                        for px in range(p):
                            out[bb, gy * g + gx, c * p * p + py * p + px] = chw[bb, c, gy * p + py, gx * p + px]
    return out.reshape(-1)


# ---- taps, vectorised (this module's own; the emulation, the census and exact_fp64 use them) ------------------------------
def _taps(n, S, defect=None, num=None):
    """i0, i1, lam and the unclamped src of every output index of an axis of n source pixels; num: the numerator of the
    scale when it is not n (the swapped-scales defect)."""
    f32 = np.float32
    d = np.arange(S, dtype=np.float32)
    if defect == "align_corners":
        raw = d * (f32(n - 1) / f32(max(S - 1, 1)))
    else:
        raw = (f32(n if num is None else num) / f32(S)) * (d + f32(0.5)) - f32(0.5)
    src = raw if defect == "no_low_clamp" else np.maximum(raw, f32(0.0))
    fl = np.floor(src).astype(np.int64)
    i0 = np.minimum(fl, n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    lam = (src - i0.astype(np.float32)).astype(np.float32)
    if defect == "lam_before_clamp":
        lam = (raw - np.floor(raw)).astype(np.float32)
    return i0, i1, lam, raw


U = 2.0 ** -24  # unit roundoff of fp32


def _gamma(k):
    return k * U / (1.0 - k * U)


def exact_fp64(case, fr=None):
    """(exact, bound): the documented taps (i0, i1, lam and the constants a, b as fp32 numbers) combined in float64, and
    the bound on |oracle - exact| per element; both flat in the output's memory order.

    In float64 the products of an fp32 weight (24 bits) with an 8-bit pixel and their sums are exact; the products of
    the row weights with those sums and the last multiply-add round at 2^-53, which is 2^-29 of the bound's unit and is
    covered by stating the bound with gamma_k = k u / (1 - k u) instead of k u.

    Derivation (u = 2^-24, every fp32 operation fl(x) = x (1 + d), |d| <= u; nothing here underflows: the smallest
    nonzero factor is a lam >= 2^-24 times a pixel >= 1):
      1 - lx              one rounding                                    -> weight (1 - lx)(1 + d1)
      (1 - lx) * p, lx*p  one rounding each                               -> each term carries <= 2 roundings
      top = sum           one rounding; all terms are >= 0, so relative errors do not amplify -> top_exact (1 + t3)
      1 - ly, * top, sum  three more in the same way                      -> val = E (1 + t6), E = exact bilinear value
      t = val * a         one more, a > 0                                 -> t = E a (1 + t7),  |t7| <= gamma_7
      out = t + b         one rounding of the result                      -> out = (t + b)(1 + d)
    so |out - (E a + b)| <= gamma_7 |E a| + u (|E a| (1 + gamma_7) + |b|).  |t + b| <= |E a|(1 + gamma_7) + |b| is used
    instead of |E a + b| so that cancellation in the last sum costs nothing in rigour.  The bound comes from this count
    alone; no observed error went into it."""
    fr = frames(case) if fr is None else fr
    B, H, W, _ = fr.shape
    S = case.S
    y0, y1, ly, _ = _taps(H, S)
    x0, x1, lx, _ = _taps(W, S)
    rgb = fr[..., ::-1].astype(np.float64)
    lx64 = lx.astype(np.float64)[None, None, :, None]
    ly64 = ly.astype(np.float64)[None, :, None, None]
    r0, r1 = rgb[:, y0], rgb[:, y1]
    top = (1.0 - lx64) * r0[:, :, x0] + lx64 * r0[:, :, x1]
    bot = (1.0 - lx64) * r1[:, :, x0] + lx64 * r1[:, :, x1]
    E = (1.0 - ly64) * top + ly64 * bot  # [B,S,S,3]
    a, b = (v.astype(np.float64) for v in consts(case))
    Ea = np.abs(E * a)
    exact = E * a + b
    bound = _gamma(7) * Ea + U * (Ea * (1.0 + _gamma(7)) + np.abs(b))

    def lay(v):
        chw = np.ascontiguousarray(v.transpose(0, 3, 1, 2))
        if case.layout == "chw":
            return chw.reshape(-1)
        p, g = case.patch, S // case.patch
        x = chw.reshape(B, 3, g, p, g, p).transpose(0, 2, 4, 1, 3, 5).reshape(B, g * g, 3 * p * p)
        out = np.zeros((B, g * g, case.k_pad), np.float64)
        out[..., : 3 * p * p] = x
        return out.reshape(-1)

    return lay(exact), lay(bound)


# ---- census ----------------------------------------------------------------------------------------------------------
def pad_mask(case, B=None) -> np.ndarray:
    """bool, flat in the output's memory order: the zero-padded columns of the patch layout."""
    n = n_out(case, B)
    if case.layout != "patches":
        return np.zeros(n, bool)
    return (np.arange(n) % case.k_pad) >= 3 * case.patch * case.patch


def census(case, want=None) -> dict:
    """Counts in the oracle's fp32 output (pad columns excluded, except where they are what is counted)."""
    want = oracle_cached(case.name) if want is None else want
    pad = pad_mask(case, want.size // n_out(case, 1))
    v = want[~pad]
    bits = v.view(np.uint32)
    if case.dtype == "bf16":
        ties = int(((bits & 0xFFFF) == 0x8000).sum())
    else:
        r = v.astype(np.float16)
        v64, r64 = v.astype(np.float64), r.astype(np.float64)
        other = np.nextafter(r, np.where(v64 > r64, np.inf, -np.inf).astype(np.float16)).astype(np.float64)
        ties = int(((v64 != r64) & (np.abs(v64 - r64) == np.abs(other - v64))).sum())
    y0, y1, _, rawy = _taps(case.H, case.S)
    x0, x1, _, rawx = _taps(case.W, case.S)
    return {
        # fp32 values in the f16 subnormal range: an f16 cast must keep them as subnormals, a bf16 cast as normal numbers
        "f16_subnormal": int(((np.abs(v) < 2.0 ** -14) & (v != 0)).sum()),
        "ties": ties,
        "plus_zero": int((bits == 0).sum()),
        "clamp_top": int((rawy < 0).sum()), "clamp_bottom": int((y0 + 1 > case.H - 1).sum()),
        "clamp_left": int((rawx < 0).sum()), "clamp_right": int((x0 + 1 > case.W - 1).sum()),
        "pad_columns": case.k_pad - 3 * case.patch * case.patch if case.layout == "patches" else 0,
    }


# ---- the kernel's arithmetic, with room for a planted defect --------------------------------------------------------------
DEFECTS = (
    "bgr_not_swapped",     # channel c read from byte c instead of 2 - c
    "align_corners",       # taps without the half-pixel offset
    "no_low_clamp",        # src < 0 not clamped to 0
    "lam_before_clamp",    # lam from the unclamped src
    "scales_swapped",      # ax and ay exchanged
    "frame_stride",        # frame b at b * S*S*3 instead of b * H*W*3
    "pyx_c_order",         # k decoded as (py, px, c) instead of (c, py, px)
    "pad_nonzero",         # pad columns hold a value
    "pad_threshold",       # pad begins one chunk late
    "fused_affine",        # val * a + b with one rounding
    "cast_rtz",            # cast rounds toward zero
    "cast_half_away",      # cast rounds ties away from zero
    "flush_subnormal",     # values in the f16 subnormal range become zero
    "minus_zero",          # +0.0 stored as -0.0
    "fast_when_h_only",    # identity fast path taken when H == S and W != S
    "fast_e7_pixel6",      # the fast path's last element of a chunk taken from pixel 6
)


def emulate(case, fr=None, defect=None) -> np.ndarray:
    """int16 bits of the whole output as csrc/context.hip computes it: thread idx -> (frame, remainder) -> per element
    (channel, oy, ox, pad) -> taps -> fp32 value -> cast.  ``defect`` plants one of DEFECTS."""
    assert defect is None or defect in DEFECTS, defect
    fr = frames(case) if fr is None else fr
    f32 = np.float32
    B, H, W, _ = fr.shape
    S, p, k_pad = case.S, case.patch, case.k_pad
    flat = fr.reshape(-1)
    a, b = consts(case)
    patches = case.layout == "patches"
    per_frame = chunks_per_frame(case)
    idx = np.arange(per_frame * B, dtype=np.int64)
    bb = idx // per_frame
    r = idx - bb * per_frame
    e = np.arange(8, dtype=np.int64)[None, :]
    if patches:
        g, pp, chunks = S // p, p * p, k_pad // 8
        pi = r // chunks
        k = ((r - pi * chunks) * 8)[:, None] + e
        pad = k >= 3 * pp + (8 if defect == "pad_threshold" else 0)
        if defect == "pyx_c_order":
            c, rem = k % 3, k // 3
        else:
            c = k // pp
            rem = k - c * pp
        py = rem // p
        px = rem - py * p
        oy = (pi // g)[:, None] * p + py
        ox = (pi % g)[:, None] * p + px
    else:
        rc = S // 8
        c1 = r // (S * rc)
        r2 = r - c1 * S * rc
        oy1 = r2 // rc
        ox = ((r2 - oy1 * rc) * 8)[:, None] + e
        c, oy = np.broadcast_to(c1[:, None], ox.shape), np.broadcast_to(oy1[:, None], ox.shape)
        pad = np.zeros(ox.shape, bool)
    c = np.minimum(c, 2)
    oy, ox = np.minimum(oy, S - 1), np.minimum(ox, S - 1)  # pad lanes only: their value is discarded
    ch = c if defect == "bgr_not_swapped" else 2 - c
    base = (bb * (S * S * 3 if defect == "frame_stride" else H * W * 3))[:, None]

    def px_at(y, x):
        return np.take(flat, base + (y * W + x) * 3 + ch, mode="clip").astype(np.float32)

    ac, bc = a[c], b[c]
    fast = is_fast(case) or (defect == "fast_when_h_only" and is_fast(case._replace(W=case.S)))
    if fast:
        oxe = ox - (e == 7) if defect == "fast_e7_pixel6" else ox
        val = px_at(oy, oxe)
    else:
        swap = defect == "scales_swapped"
        y0, y1, ly, _ = _taps(H, S, defect, num=W if swap else H)
        x0, x1, lx, _ = _taps(W, S, defect, num=H if swap else W)
        ly, lx = ly[oy], lx[ox]
        one = f32(1.0)
        top = (one - lx) * px_at(y0[oy], x0[ox]) + lx * px_at(y0[oy], x1[ox])
        bot = (one - lx) * px_at(y1[oy], x0[ox]) + lx * px_at(y1[oy], x1[ox])
        val = (one - ly) * top + ly * bot
    if defect == "fused_affine":
        v = (val.astype(np.float64) * ac.astype(np.float64) + bc.astype(np.float64)).astype(np.float32)
    else:
        v = val * ac + bc
    assert v.dtype == np.float32
    if defect == "flush_subnormal":
        v = np.where(np.abs(v) < f32(2.0 ** -14), np.copysign(f32(0.0), v), v)
    mode = {"cast_rtz": "rtz", "cast_half_away": "half_away"}.get(defect, "rne")
    out = bits16(v, case.dtype, mode).copy()
    if defect == "minus_zero":
        out[out == 0] = np.int16(-0x8000)
    out[pad] = bits16(bc, case.dtype)[pad] if defect == "pad_nonzero" else 0
    return out.reshape(-1)

