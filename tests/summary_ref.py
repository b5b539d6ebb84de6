"""Test oracle of the group summaries (include/vidmem.h vm_memory_summaries).

A group is a maximal run of consecutive live rows with one key.  Its centroid: fp64 vector adds of the rows strictly in
row order (``S = S + x`` per row, never ``np.sum``), ``N`` from a sequential ``np.cumsum`` of the squares, one division,
and ONE rounding to the 16-bit format - ``astype(np.float16)`` for fp16 (numpy rounds once), a written-out
round-to-nearest-even on the fp64 bits for bf16.  Key scores: ``oracle.cref.cosine_matrix`` (the exact C restatement of
the reference cosine) of the stored centroid row against the group's rows; the key row by (score desc, row asc).
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from oracle import cref


def to_f64(bits, dtype) -> np.ndarray:
    """uint16 bit patterns -> their exact values in fp64."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if dtype == "f16":
        return bits.view(np.float16).astype(np.float64)
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def _round_bf16(x) -> np.ndarray:
    """fp64 -> bf16 bits, one round-to-nearest-even on the integer bits of the double."""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    one = np.uint64(1)
    sign = ((u >> np.uint64(48)) & np.uint64(0x8000))
    ef = ((u >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64)
    frac = u & ((one << np.uint64(52)) - one)
    e = ef - 1023
    sig = frac | (one << np.uint64(52))
    shift = 45 + np.maximum(0, -126 - e)
    tiny = (ef == 0) | (shift > 54)                      # zero, an fp64 subnormal, or below half the smallest subnormal
    sh = np.minimum(shift, 54).astype(np.uint64)
    q = sig >> sh
    rem = sig & ((one << sh) - one)
    half = one << (sh - one)
    q = q + ((rem > half) | ((rem == half) & ((q & one) == one))).astype(np.uint64)
    normal = ((np.maximum(e, -126) + 127).astype(np.uint64) << np.uint64(7)) + q - np.uint64(128)
    mag = np.where(e >= -126, normal, q)
    mag = np.where(tiny, np.uint64(0), mag)
    mag = np.minimum(mag, np.uint64(0x7f80))             # overflow: infinity
    nan = (ef == 0x7ff) & (frac != 0)
    mag = np.where(ef == 0x7ff, np.where(nan, np.uint64(0x7fc0), np.uint64(0x7f80)), mag)
    return (sign | mag).astype(np.uint16)


def round16(x, dtype) -> np.ndarray:
    """fp64 -> the bits of the nearest 16-bit value, ties to even, rounded ONCE."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    return _round_bf16(x)


def row_sums(bits, dtype, reverse=False) -> np.ndarray:
    """S [D]: the rows added one by one in row order (``reverse``: in the opposite order), from 0.0."""
    x = to_f64(bits, dtype)
    S = np.zeros(x.shape[1], np.float64)
    for r in (range(x.shape[0] - 1, -1, -1) if reverse else range(x.shape[0])):
        S = S + x[r]
    return S


def centroid(bits, dtype, reverse=False) -> np.ndarray:
    """uint16 [D]: the centroid row of one group (``bits`` [rows, D] in row order)."""
    S = row_sums(bits, dtype, reverse)
    N = np.sqrt(np.cumsum(S * S)[-1])                    # cumsum adds left to right, one rounding per partial sum
    if N == 0.0:
        return np.zeros(S.size, np.uint16)
    return round16(S / N, dtype)


class Summary(NamedTuple):
    first_rows: np.ndarray    # int64 [G] row ids
    n_rows: np.ndarray        # int64 [G]
    keys: np.ndarray          # int64 [G]
    centroids: np.ndarray     # uint16 [G, D]
    key_rows: np.ndarray      # int64 [G]
    key_scores: np.ndarray    # float64 [G]


def summarize(bits, keys, dtype, base=0) -> Summary:
    """Every group of the live rows ``bits`` [n, D] (row-id order, first row id ``base``) with group keys ``keys`` [n]."""
    bits = np.ascontiguousarray(bits)
    keys = np.asarray(keys, np.int64)
    n, D = bits.shape
    starts = np.concatenate([[0], np.nonzero(keys[1:] != keys[:-1])[0] + 1]) if n else np.zeros(0, np.int64)
    ends = np.concatenate([starts[1:], [n]]) if n else starts
    G = len(starts)
    cents = np.zeros((G, D), np.uint16)
    key_rows, key_scores = np.zeros(G, np.int64), np.zeros(G, np.float64)
    for g, (a, b) in enumerate(zip(starts.tolist(), ends.tolist())):
        cents[g] = centroid(bits[a:b], dtype)
        score = cref.cosine_matrix(cents[g:g + 1], np.ascontiguousarray(bits[a:b]), dtype=dtype)[0]
        best = int(np.argmax(score))                     # argmax keeps the first = lowest row on ties
        key_rows[g], key_scores[g] = base + a + best, score[best]
    return Summary(base + starts.astype(np.int64), (ends - starts).astype(np.int64), keys[starts] if n else keys[:0],
                   cents, key_rows, key_scores)


def window(s: Summary, first_group, max_groups, D) -> Summary:
    """What a call with this window writes: slots 0 .. max_groups - 1, padded with -1 / 0.0 / zero rows."""
    g0 = max(int(first_group), 0)
    part = [x[g0:g0 + max_groups] for x in s]
    m = part[0].shape[0]
    pad = lambda x, fill: np.concatenate([x, np.full((max_groups - m,) + x.shape[1:], fill, x.dtype)])
    return Summary(pad(part[0], -1), pad(part[1], -1), pad(part[2], -1), pad(part[3].reshape(m, D), 0),
                   pad(part[4], -1), pad(part[5], 0.0))


# ---- the special groups of the tests, D = 128 ------------------------------------------------------------------------
def f64_to_bits(x, dtype) -> np.ndarray:
    return round16(np.asarray(x, np.float64), dtype)


@functools.lru_cache(maxsize=None)
def order_sensitive_bf16(D=128):
    """bf16 rows [9, D] whose exponents span 2^-60 .. 2^60: row 0 is small, rows 1 and 2 are +B and -B with B around
    2^50 .. 2^60, the rest random.  In row order the small row is absorbed by B before B cancels; in the opposite order
    B cancels first and the small row survives: the sum depends on the order."""
    rng = np.random.default_rng(77)
    mant = lambda shape: 1.0 + rng.integers(0, 128, shape) / 128.0
    sgn = lambda shape: rng.choice([-1.0, 1.0], shape)
    small = sgn(D) * mant(D) * 2.0 ** rng.integers(-10, 11, D)
    big = sgn(D) * mant(D) * 2.0 ** rng.integers(50, 61, D)
    rest = sgn((6, D)) * mant((6, D)) * 2.0 ** rng.integers(-60, -20, (6, D))
    bits = f64_to_bits(np.vstack([small, big, -big, rest]), "bf16")
    bits.setflags(write=False)
    return bits


def special_groups(dtype, D=128):
    """[(name, bits [rows, D])]: the special groups of the issue, in the memory's dtype."""
    rng = np.random.default_rng(5 if dtype == "f16" else 6)
    x = f64_to_bits(rng.standard_normal(D), dtype)
    tiny = 2.0 ** (-24 if dtype == "f16" else -133)          # the smallest subnormal of the format
    sub = f64_to_bits(rng.integers(-40, 41, D) * tiny, dtype)
    sub[:4] = f64_to_bits(np.array([1.0, -1.0, 0.5, 2.0 ** -10]), dtype)     # a few normal values among them
    out = [("zeros", np.zeros((3, D), np.uint16)),
           ("cancel", np.stack([x, x ^ np.uint16(0x8000)])),
           ("identical", np.tile(f64_to_bits(rng.standard_normal(D), dtype), (5, 1))),
           ("subnormal", sub[None, :].copy()),
           ("all_subnormal", f64_to_bits(rng.integers(-40, 41, (2, D)) * tiny, dtype))]
    if dtype == "bf16":
        out.append(("order", np.array(order_sensitive_bf16(D))))
    return out
