"""Test helper: memories and queries OUTSIDE unit norm, for the domain of the top-k certificate (DESIGN.md 4.1,
csrc/topk_common.h cert_eps).  A plain module, not a conftest.

Three things:
  * ``scaled``    - 16-bit rows times per-row powers of two, and whether that scaling was EXACT.  Exactly scaled rows and
                    queries leave the reference cosine bit-identical: every product and every partial sum of the dot
                    and of the norms moves by one power of two (fp64 has the exponent room), sqrt and the division
                    included.  So an exact class has a second expectation that shares no code with any kernel: the
                    answer of the unscaled memory to the unscaled queries.
  * ``standin``   - a numpy stand-in for what the fp32 scan's arithmetic can deliver (fp32 products and partial sums,
                    left to right, no fma, times fp32(1 / norm)): good enough to show that a class is inside or outside
                    the certificate's domain, no model of the matrix unit's summation order.
  * ``CLASSES`` / ``DomainSet`` - the classes and their data: unit rows rounded to 16 bits with the plants the other
                    top-k scenarios have (a near-duplicate pair per probe query, an exact duplicate pair, a zero row, a
                    zero query), then scaled.

Constants that differ from the first sketch of the classes, each moved because its precondition failed on the CPU
(tests/test_domain_cpu.py asserts the preconditions):
  * bf16_under scales by 2^-70, not 2^-60: at 2^-60 the products of two unit rows' elements (~2^-128) are fp32
    subnormals that still carry some 20 bits, and the stand-in - numpy keeps subnormals - stays within the bound.  At
    2^-70 the products are at most a bit or two above 2^-149: outside with or without flush-to-zero.
  * the fp16 base rows sit on the grid 2^-16, so that the factor 2^-8 of f16_mixed lands every element on an fp16
    subnormal step (2^-24) and the scaling is exact as the class demands.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from tests.support import TD, bits  # noqa: F401  (DR.bits for the tests)


def cert_eps(D: int) -> float:
    """csrc/topk_common.h cert_eps: 2 (D + 8) 2^-24."""
    return 2.0 * (D + 8) * 2.0 ** -24


# the norm interval of the certificate's domain (csrc/topk_common.h VM_CERT_NORM_MIN / MAX)
NORM_MIN, NORM_MAX = 2.0 ** -40, 2.0 ** 40


def scaled(rows16: torch.Tensor, exps) -> Tuple[torch.Tensor, bool]:
    """rows16 [n, D] (fp16 / bf16) times 2^exps[row], computed with ldexp in fp32 and cast back -> (rows, exact).
    exact: the round trip ldexp(., -e) reproduces the input bit for bit and nothing overflowed - no element lost a bit
    to a subnormal or to the cast."""
    e = torch.as_tensor(exps, dtype=torch.int32, device=rows16.device).reshape(-1, 1)
    out = torch.ldexp(rows16.float(), e).to(rows16.dtype)
    back = torch.ldexp(out.float(), -e).to(rows16.dtype)
    exact = bool(torch.isfinite(out.float()).all()) and torch.equal(back.view(torch.int16), rows16.view(torch.int16))
    return out, exact


def as_f64(b: np.ndarray, dtype: str) -> np.ndarray:
    """uint16 bit patterns -> float64 values."""
    if dtype == "f16":
        return b.view(np.float16).astype(np.float64)
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def standin(qbits: np.ndarray, rbits: np.ndarray, dtype: str) -> np.ndarray:
    """[Q, n] fp32: for every pair the fp32 left-to-right dot (one rounding per product and per partial sum) times
    fp32(1 / ||row||), 0 for a zero row - the scan's score before the division by ||q||."""
    q = as_f64(qbits, dtype).astype(np.float32)
    r = as_f64(rbits, dtype).astype(np.float32)
    acc = np.zeros((q.shape[0], r.shape[0]), np.float32)
    with np.errstate(all="ignore"):
        for i in range(q.shape[1]):
            acc = acc + q[:, i:i + 1] * r[None, :, i]
        norm = np.sqrt((as_f64(rbits, dtype) ** 2).sum(1))
        rn = np.where(norm > 0, 1.0 / np.where(norm > 0, norm, 1.0), 0.0).astype(np.float32)
        return acc * rn[None, :]


def norms(b: np.ndarray, dtype: str) -> np.ndarray:
    with np.errstate(all="ignore"):
        return np.sqrt((as_f64(b, dtype) ** 2).sum(1))


@dataclass(frozen=True)
class DomainClass:
    name: str
    dtype: str
    row_exp: Tuple[int, int]      # per-row exponent, uniform in [lo, hi]
    query_exp: Tuple[int, int]
    exact: bool                   # the scaling is exact: the unscaled answer is a second expectation
    inside: bool                  # inside the certificate's domain: nothing but the zero query may be flagged
    rnorm_plants: bool = False    # bf16_rnorm: rows whose fp32 reciprocal norm is not a normal number


CLASSES = {c.name: c for c in (
    DomainClass("f16_high", "f16", (17, 17), (17, 17), True, True),
    DomainClass("f16_mixed", "f16", (-8, 17), (-8, 17), True, True),
    DomainClass("f16_subnormal", "f16", (-14, -14), (-14, -14), False, True),   # inside iff the MFMA keeps subnormals
    DomainClass("bf16_mixed", "bf16", (-30, 30), (-30, 30), True, True),
    DomainClass("bf16_under", "bf16", (-70, -70), (-70, -70), True, False),
    DomainClass("bf16_over", "bf16", (50, 50), (80, 80), True, False),
    DomainClass("bf16_rnorm", "bf16", (0, 0), (0, 0), False, False, rnorm_plants=True),
)}
EXACT = [c.name for c in CLASSES.values() if c.exact]
INSIDE = [c.name for c in CLASSES.values() if c.inside]
OUTSIDE = [c.name for c in CLASSES.values() if not c.inside]


def _unit16(x: torch.Tensor, dtype: str) -> torch.Tensor:
    x = x / x.norm(dim=1, keepdim=True).clamp_min(1e-6)
    if dtype == "f16":   # the grid 2^-16: every element times 2^-8 is a whole number of fp16 subnormal steps
        x = torch.round(x * 65536.0) / 65536.0
    return x.to(TD[dtype])


class DomainSet:
    """The data of one class: ``base`` rows (unit, 16-bit, planted) and ``rows`` = the same rows scaled, both [n, D];
    ``queries(Q)`` likewise.  ``pairs`` = the planted near-duplicate pairs as (row - 1, row); ``dup`` = the exact
    duplicate pair; ``zero_row``.  bf16_rnorm replaces rows near the front by its plants after the scaling."""

    def __init__(self, cls: DomainClass, n: int, D: int, seed: int, device="cpu", pair_at: Optional[List[int]] = None,
                 base: Optional[torch.Tensor] = None):
        """base: rows to start from instead of random ones (the range tests' clustered rows); they are normalised,
        rounded and planted as the random ones are."""
        self.cls, self.n, self.D, self.device = cls, n, D, device
        g = torch.Generator(device=device).manual_seed(seed)
        base = torch.randn((n, D), generator=g, device=device) if base is None else base.float().clone()
        self.pairs, self.centres = [], []
        used = set()
        for p in (pair_at if pair_at is not None else [n // 2]):
            if 1 <= p < n and p not in used and p - 1 not in used:
                c = torch.randn((D,), generator=g, device=device)
                for s in (p - 1, p):
                    base[s] = c + 0.05 * torch.randn((D,), generator=g, device=device)
                    used.add(s)
                self.pairs.append((p - 1, p))
                self.centres.append(c)
        base = _unit16(base, cls.dtype)
        self.dup = self.zero_row = None
        if n >= 64:
            a, b = 7, n - 9
            base[b] = base[a]
            self.dup = (a, b)
            self.zero_row = n // 3
            base[self.zero_row] = 0
        self.base = base
        lo, hi = cls.row_exp
        self.row_exps = torch.randint(lo, hi + 1, (n,), generator=g, device=device, dtype=torch.int32)
        if self.dup:    # an exact duplicate stays one: both copies get one exponent
            self.row_exps[self.dup[1]] = self.row_exps[self.dup[0]]
        self.rows, self.rows_exact = scaled(base, self.row_exps)
        self.rnorm_rows: List[int] = []
        self.big_rows: List[int] = []

    def queries(self, Q: int, seed: int, near: bool = False):
        """-> (base queries, scaled queries, exact, picks, zero position).  The probes (one per planted pair, then the
        duplicate's row) come first, a zero query sits in the middle, the rest is random; all unit before the scaling.
        picks: up to 8 positions for the C oracle - the probes, the zero query, the last query."""
        cls, D, dev = self.cls, self.D, self.device
        g = torch.Generator(device=dev).manual_seed(seed)
        q = torch.randn((Q, D), generator=g, device=dev)
        if near:    # stored rows plus 0.1 noise, as the clustered tests' queries
            pick = torch.randint(0, self.n, (Q,), generator=g, device=dev)
            q = self.base[pick].float() + 0.1 * q
        zero = Q // 2 if Q >= 3 else None
        slots = [i for i in range(Q) if i != zero]
        probes = [c + 0.05 * torch.randn((D,), generator=g, device=dev) for c in self.centres]
        if self.dup:
            probes.insert(0, self.base[self.dup[0]].float())
        for pos, v in zip(slots, probes):
            q[pos] = v
        qb = _unit16(q, cls.dtype)
        if zero is not None:
            qb[zero] = 0
        lo, hi = cls.query_exp
        e = torch.randint(lo, hi + 1, (Q,), generator=g, device=dev, dtype=torch.int32)
        if cls.rnorm_plants and self.big_rows and len(slots) > 1:
            e[slots[1 if self.dup else 0]] = 10      # the query of the 2^125 plants, also times 2^10
        qs, exact = scaled(qb, e)
        n_probe = min(len(probes), 5)
        picks = sorted(set(slots[:n_probe] + ([zero] if zero is not None else []) + [Q - 1]))[:8]
        return qb, qs, exact, picks, zero

    def plant_rnorm(self):
        """bf16_rnorm: one-hot rows whose single element is 2^-130 (norm 2^-130, fp32 reciprocal inf) in the OLDEST
        slots - where the zero query's answer lives - and copies of the first pair's rows times 2^125 (their fp32
        reciprocal norm 2^-125 is still normal; with their query at 2^10 the fp32 dot overflows)."""
        assert self.cls.rnorm_plants
        tiny = torch.tensor(2.0 ** -130, dtype=torch.float32).to(torch.bfloat16)
        assert float(tiny.float()) == 2.0 ** -130
        for j, r in enumerate((0, 1, 2, 40)):
            self.rows[r] = 0
            self.rows[r, (3 + 5 * j) % self.D] = tiny
            self.rnorm_rows.append(r)
        a, b = self.pairs[0] if self.pairs else (10, 11)      # no pair planted: two rows of one cluster
        for j, r in enumerate((50, self.n - 20)):
            big, ok = scaled(self.base[(a, b)[j]][None], [125])
            assert ok
            self.rows[r] = big[0]
            self.big_rows.append(r)
        return self


def domain_set(name: str, n: int, D: int, seed: int, device="cpu", pair_at=None, base=None) -> DomainSet:
    ds = DomainSet(CLASSES[name], n, D, seed, device, pair_at, base)
    if CLASSES[name].rnorm_plants:
        ds.plant_rnorm()
    return ds
