"""GPU: every path of the cosine top-k (csrc/topk.hip, topk_emit.hip, topk_gscan.hip, topk_exact.hip) pinned to the
C oracle, on fresh, half-filled and wrapped memories.

Every case names the path it takes (tests/topk_plan.py, the dispatch's mirror) and asserts that one call launches
exactly the mirror's kernels, so a retuned dispatch rule fails here instead of quietly moving the case off its path.
Then: the fast path without the redo - every query it did not flag equals the exhaustive kernel bit for bit (the
certification claim itself); with the redo, every query; and up to 8 queries - the planted ones, the zero query, the
last query of a ragged group - against the C oracle, the one reference that shares no code with the kernels.

Memories are built on the device from a seeded generator, appended in uneven chunks, with planted rows: near-duplicate
pairs of a query on both sides of every pass limit and of the dense range's edges, an exact duplicate pair with one
copy inside the dense range and one outside it, and a zero row (plus a zero query).
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import pytest
import torch

from tests import support
from tests import topk_plan as TP
from tests.support import TD, bits
from tests.topk_ref import oracle_rows_parallel

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
CHUNKS = (977, 20_011, 4_099, 31_337, 12_289, 65_521)   # uneven append sizes, cycled


@dataclass(frozen=True)
class MemSpec:
    """How a case's memory is built: ``total`` rows appended to a memory of ``cap`` rows (a ring wraps past it)."""
    dtype: str
    D: int
    cap: int
    total: int
    ring: bool = False
    seed: int = 0

    @property
    def n(self) -> int:
        return min(self.total, self.cap)

    @property
    def head(self) -> int:
        return self.total % self.cap if self.ring and self.total > self.cap else 0

    @property
    def base(self) -> int:
        return self.total - self.n

    def row_of_slot(self, p: int) -> int:
        """Row id (index of the appended history) stored in physical slot p."""
        return self.base + (p - self.head) % self.cap if self.ring and self.total > self.cap else p

    def tag(self) -> str:
        fill = f"ring{self.total}" if self.ring else f"n{self.total}"
        return f"{self.dtype}-D{self.D}-cap{self.cap}-{fill}"


@dataclass(frozen=True)
class Case:
    table: str
    mem: MemSpec
    Q: int
    k: int

    def plan(self, num_cus: int = 256) -> TP.Plan:
        return TP.plan(self.Q, self.k, self.mem.D, self.mem.dtype, self.mem.cap, num_cus)

    @property
    def id(self) -> str:
        p = self.plan()
        path = p.family
        if p.family in ("list", "list+prepass"):
            path += f"-KL{p.KL}-QT{p.QT}"
        elif p.family == "cascade":
            path += f"-KS{p.KS}-NG{p.NG}-" + "".join("g" if x.kind == "gscan" else "e" for x in p.passes[1:])
        return f"{self.table}-{path}-{self.mem.tag()}-Q{self.Q}-k{self.k}"


# ---------------------------------------------------------------------------------------------------------------------
# the case table (tests/test_topk_plan_cpu.py feeds it through the mirror: every instantiation must be reached)
# ---------------------------------------------------------------------------------------------------------------------
def _table_a():
    """Few queries at k >= 11 on a wrapped 100k ring (the cascade for KL >= 32, i.e. k >= 13; k = 11 is KL = 16)."""
    out = []
    for dtype, D in (("f16", 768), ("bf16", 1024)):
        mem = MemSpec(dtype, D, 100_000, 161_337, ring=True, seed=11 + D)
        for Q, k in ((1, 11), (1, 20), (16, 20), (48, 32), (5, 58)):
            out.append(Case("A", mem, Q, k))
    return out


def _table_b():
    """Every emit instantiation: KS in {1, 2, 4, 6, 8} x dtype, NG = 1 (49..128 queries) and NG = 2 (129..256)."""
    out = []
    ng1_q, ng2_q, ks_k = (49, 77, 100, 128, 64), (129, 200, 256, 173), (10, 5, 20, 12, 30)
    for dtype in ("f16", "bf16"):
        for i, ks in enumerate((1, 2, 4, 6, 8)):
            D = 128 * ks
            mem = (MemSpec(dtype, D, 100_000, 100_000 + 54_321, ring=True, seed=20 + ks) if dtype == "f16"
                   else MemSpec(dtype, D, 100_000, 97_003, seed=30 + ks))
            out.append(Case("B", mem, ng1_q[i], ks_k[i]))
            if ks <= 6:
                out.append(Case("B", mem, ng2_q[i], ks_k[(i + 2) % 5]))
    return out


def _table_c():
    """GEMM-class scan: 300 / 600 queries on a 300k memory (only the pass over [32,768, 262,144) has the tiles), and
    1,024 queries on a 100k memory (pass 1 emit, pass 2 gscan)."""
    out = []
    for dtype in ("f16", "bf16"):
        for D in (256, 1024):
            mem = (MemSpec(dtype, D, 300_000, 299_555, seed=40 + D) if dtype == "f16"
                   else MemSpec(dtype, D, 300_000, 300_000 + 123_457, ring=True, seed=50 + D))
            for Q in (300, 600):
                out.append(Case("C", mem, Q, 10 if Q == 300 else 20))
    for dtype in ("f16", "bf16"):
        for D in (256, 1024):
            mem = (MemSpec(dtype, D, 100_000, 99_001, seed=60 + D) if dtype == "f16"
                   else MemSpec(dtype, D, 100_000, 100_000 + 33_333, ring=True, seed=70 + D))
            out.append(Case("C", mem, 1024, 10))
    return out


# (KL, QT) -> (Q, k): every list-scan instantiation, ragged query counts
LIST_PAIRS = {(8, 1): (1, 6), (8, 2): (17, 3), (8, 4): (49, 1), (16, 1): (16, 7), (16, 2): (33, 12),
              (16, 4): (100, 10), (32, 1): (5, 13), (32, 2): (47, 26), (64, 1): (70, 27)}


def _table_d():
    out = []
    mems = {"f16": MemSpec("f16", 256, 60_000, 59_999, seed=80),
            "bf16": MemSpec("bf16", 640, 60_000, 60_000 + 7_777, ring=True, seed=81)}
    for dtype in ("f16", "bf16"):
        for (Q, k) in LIST_PAIRS.values():
            out.append(Case("D", mems[dtype], Q, k))
    # the sampled pre-pass: 17..48 queries, k <= 10, a 100k memory
    out.append(Case("D", MemSpec("f16", 512, 100_000, 100_000 + 41_000, ring=True, seed=82), 33, 10))
    out.append(Case("D", MemSpec("bf16", 768, 100_000, 88_888, seed=83), 40, 4))
    # D outside the emit set: the list scan with the pre-pass at QT 4 or (LDS-limited) 2
    for dtype, D, total, ring in (("f16", 384, 100_000, False), ("bf16", 1280, 100_000 + 9_999, True),
                                  ("f16", 2048, 95_000, False)):
        mem = MemSpec(dtype, D, 100_000, total, ring=ring, seed=84 + D)
        for Q in (64, 200):
            out.append(Case("D", mem, Q, 10))
    # bf16 finalize with (D = 512) and without (D = 1024) the candidate rows staged in LDS, KL = 64
    out.append(Case("D", MemSpec("bf16", 512, 60_000, 52_345, seed=85), 20, 40))
    out.append(Case("D", MemSpec("bf16", 1024, 60_000, 60_000 + 5_000, ring=True, seed=86), 20, 40))
    return out


FILL_LEVELS = (0, 1, "k-1", 4_095, 4_096, 4_097, 16_383, 16_385, 32_767, 32_800, 131_100)
E_FAMILIES = {"list": ("f16", 5, 5), "prepass": ("bf16", 40, 10), "cascade-few": ("f16", 16, 20),
              "cascade-many": ("bf16", 300, 10)}


def _table_e():
    """A growing memory (not a ring) at every fill level that moves the dense range across a pass limit."""
    out = []
    for cap in (100_000, 300_000):
        for fam, (dtype, Q, k) in E_FAMILIES.items():
            for lvl in FILL_LEVELS:
                n = k - 1 if lvl == "k-1" else lvl
                if n <= cap:
                    out.append(Case("E", MemSpec(dtype, 256, cap, n, seed=90 + n % 97), Q, k))
    return out


RING_HEADS = ("0-after-2-wraps", 1, 255, 256, 3_839, 3_840, 4_095, 4_096, 32_767, 32_769, 99_999)


def _table_f():
    out = []
    cap = 100_000
    for h in RING_HEADS:
        total = 2 * cap if h == "0-after-2-wraps" else cap + h
        out.append(Case("F", MemSpec("f16", 256, cap, total, ring=True, seed=100), 16, 20))
        out.append(Case("F", MemSpec("bf16", 256, cap, total, ring=True, seed=101), 200, 10))
    return out


def _table_h():
    """k > 58: the exhaustive kernel is the only route (also for k > n)."""
    out = []
    for dtype, D in (("f16", 768), ("bf16", 1024)):
        mem = MemSpec(dtype, D, 100_000, 20_000, seed=110 + D)
        for k in (59, 64, 100, 300):
            out.append(Case("H", mem, 8, k))
        out.append(Case("H", MemSpec(dtype, D, 100_000, 150, seed=120 + D), 8, 300))
    return out


CASES_A, CASES_B, CASES_C, CASES_D = _table_a(), _table_b(), _table_c(), _table_d()
CASES_E, CASES_F, CASES_H = _table_e(), _table_f(), _table_h()
CASES = CASES_A + CASES_B + CASES_C + CASES_D + CASES_E + CASES_F + CASES_H
# min_score x score_mode: one case each of A - D
G_BASE = {"A": next(c for c in CASES_A if (c.Q, c.k, c.mem.dtype) == (16, 20, "f16")),
          "B": next(c for c in CASES_B if c.plan().NG == 2 and c.mem.dtype == "bf16"),
          "C": next(c for c in CASES_C if c.mem.cap == 300_000 and c.mem.dtype == "f16"),
          "D": next(c for c in CASES_D if c.plan().family == "list+prepass")}
G_THRESHOLDS = ("inside", "above-all", "below-all")


# ---------------------------------------------------------------------------------------------------------------------
# memories
# ---------------------------------------------------------------------------------------------------------------------
class Scenario:
    """A built memory, the host bit patterns of its searchable rows (row-id order) and its planted probes."""

    def __init__(self, spec: MemSpec):
        from vidmem.memory import EmbeddingMemory
        self.spec = spec
        D, n, total = spec.D, spec.n, spec.total
        g = torch.Generator(device="cuda").manual_seed(1000 + spec.seed)
        hist = torch.randn((max(total, 1), D), generator=g, device="cuda", dtype=torch.float32)[:total]
        self.probes = []          # (query vector fp32, expected first two row ids or None)
        used = set()

        def free(p):
            return 0 <= p < n and p not in used

        # near-duplicate pairs at (p - 1, p) for every limit a path cuts the rows at and the dense range's edges
        d0, d1 = TP.dense_range(n, spec.head)
        edges = sorted({d0, d1, TP.EMIT_CAP, TP.SAMPLE_ROWS, 32_768, 131_072, 262_144})
        for p in edges:
            if free(p - 1) and free(p):
                c = torch.randn((D,), generator=g, device="cuda")
                for s in (p - 1, p):
                    hist[spec.row_of_slot(s)] = c + 0.05 * torch.randn((D,), generator=g, device="cuda")
                    used.add(s)
                self.probes.append((c + 0.05 * torch.randn((D,), generator=g, device="cuda"), None))
        hist = hist / hist.norm(dim=1, keepdim=True).clamp_min(1e-6)
        # an exact duplicate pair: one copy inside the dense range, one outside
        dup = None
        inside = d0 + 1
        outside = next((s for s in (d0 - 7, d1 + 7, d1 + 300) if free(s) and not d0 <= s < d1), None)
        if free(inside) and outside is not None:
            a, b = spec.row_of_slot(inside), spec.row_of_slot(outside)
            hist[b] = hist[a]
            used.update((inside, outside))
            dup = (min(a, b), max(a, b))
        # a zero row
        zero = next((s for s in (n // 3, n // 3 + 1, n // 3 + 2) if free(s)), None)
        if zero is not None:
            hist[spec.row_of_slot(zero)] = 0
            used.add(zero)
        rows = hist.to(TD[spec.dtype])
        if dup is not None:
            self.probes.insert(0, (rows[dup[0]].float(), dup))
        self.mem = EmbeddingMemory(spec.cap, D, spec.dtype, ring=spec.ring)
        lo, i = 0, 0
        while lo < total:
            step = CHUNKS[i % len(CHUNKS)]
            self.mem.append(rows[lo:lo + step])
            lo, i = lo + step, i + 1
        assert len(self.mem) == total
        self.live = bits(rows[spec.base:]) if n else np.zeros((0, D), np.uint16)
        del hist, rows

    def queries(self, Q: int, seed: int):
        """Q queries: the probes first (the duplicate pair's query at 0), a zero query in the middle, random rest;
        -> (queries, {position: expected first two rows}, oracle picks, position of the zero query or None)."""
        D = self.spec.D
        g = torch.Generator(device="cuda").manual_seed(seed)
        q = torch.randn((Q, D), generator=g, device="cuda", dtype=torch.float32)
        zero = Q // 2 if Q >= 3 else None
        slots = [i for i in range(Q) if i != zero]
        expect = {}
        for pos, (v, want) in zip(slots, self.probes):
            q[pos] = v
            if want is not None:
                expect[pos] = want
        if zero is not None:
            q[zero] = 0
        picks = slots[:min(len(self.probes), 5)] + ([zero] if zero is not None else []) + [Q - 1]
        return q.to(TD[self.spec.dtype]), expect, sorted(set(picks))[:8], zero

    def close(self):
        self.mem.close()


_cache = {}


def scenario(spec: MemSpec) -> Scenario:
    """The memory of one spec, kept while consecutive cases search it (one at a time: they are large)."""
    if spec not in _cache:
        for old in _cache.values():
            old.close()
        _cache.clear()
        torch.cuda.empty_cache()
        _cache[spec] = Scenario(spec)
    return _cache[spec]


@pytest.fixture(scope="module", autouse=True)
def _report():
    """Highest number of queries the fast path flagged, per table and family (printed with -s)."""
    yield
    for sc in _cache.values():
        sc.close()
    _cache.clear()
    for key in sorted(FLAGGED):
        print(f"\n[topk paths] most queries flagged in one call, {key}: {FLAGGED[key]}")


FLAGGED = {}


# ---------------------------------------------------------------------------------------------------------------------
# the check
# ---------------------------------------------------------------------------------------------------------------------
def _same(a_s, a_r, b_s, b_r) -> bool:
    return np.array_equal(a_r, b_r) and np.array_equal(a_s.view(np.int64), b_s.view(np.int64))


def _sanity(s, r, n, k, filtered):
    for i in range(r.shape[0]):
        live = r[i][r[i] >= 0]
        assert len(set(live.tolist())) == live.size, f"query {i}: a row id repeats {r[i]}"
        m = live.size
        assert (r[i, m:] == -1).all() and (s[i, m:] == 0.0).all(), f"query {i}: padding {r[i]} {s[i]}"
        if not filtered:
            assert m == min(n, k), f"query {i}: {m} results of {min(n, k)}"


def run_case(case: Case, score_mode: int = 0, thr: Optional[str] = None):
    from vidmem.memory import TopkScratch
    spec, Q, k = case.mem, case.Q, case.k
    sc = scenario(spec)
    mem = sc.mem
    q, expect, picks, zero = sc.queries(Q, seed=Q * 7919 + k)
    plan = case.plan(torch.cuda.get_device_properties(0).multi_processor_count)
    kw = dict(score_mode=score_mode)
    if thr is not None:
        if thr == "inside":   # a threshold inside the top-k: the median of the exact k/2-th returned scores
            es, _ = mem.topk(q, k, exact=True, score_mode=score_mode)
            col = es.cpu().numpy()[:, k // 2]
            kw["min_score"] = float(np.median(col))
        else:
            kw["min_score"] = 1.5 if thr == "above-all" else (-1.5 if score_mode == 0 else -0.5)
    es, er = mem.topk(q, k, exact=True, **kw)
    es, er = es.cpu().numpy(), er.cpu().numpy()

    if plan.family == "exact":
        (s1, r1), launches = support.launches(mem, lambda: mem.topk(q, k, **kw))
        assert launches["topk_scan"] == 0 and launches["topk_finalize"] == 0 and launches["topk_exact"] >= 1, launches
        s1, r1 = s1.cpu().numpy(), r1.cpu().numpy()
        assert _same(s1, r1, es, er)
    else:
        scratch = TopkScratch.for_(mem, Q, k)
        (s0, r0), launches = support.launches(mem, lambda: mem.topk(q, k, redo=False, scratch=scratch, **kw))
        want = (plan.launches["topk_scan"], plan.launches["topk_finalize"])
        assert (launches["topk_scan"], launches["topk_finalize"]) == want, (plan.family, launches, want)
        flags = scratch.flags[:Q].cpu().numpy()
        s0, r0 = s0.cpu().numpy(), r0.cpu().numpy()
        ok = flags == 0
        bad = np.flatnonzero(ok & ~((r0 == er).all(1) & (s0.view(np.int64) == es.view(np.int64)).all(1)))
        assert bad.size == 0, f"certified (unflagged) queries differ from the exhaustive answer: {bad[:8]}"
        flagged = int((~ok).sum())
        key = f"{case.table} {plan.family}" + (" min_score" if thr else "")
        FLAGGED[key] = max(FLAGGED.get(key, 0), flagged)
        if thr is None:   # only the zero query (its every score ties) may need the redo
            assert set(np.flatnonzero(flags).tolist()) <= {zero}, (np.flatnonzero(flags)[:8], flags[flags != 0][:8], zero)
        scratch.uncert.zero_()
        s1, r1 = mem.topk(q, k, scratch=scratch, **kw)
        s1, r1 = s1.cpu().numpy(), r1.cpu().numpy()
        bad = np.flatnonzero(~((r1 == er).all(1) & (s1.view(np.int64) == es.view(np.int64)).all(1)))
        assert bad.size == 0, f"queries differ from the exhaustive answer after the redo: {bad[:8]}"
    want_r, want_s = oracle_rows_parallel(bits(q), sc.live, k, spec.dtype, picks, threads=THREADS, **kw)
    want_r = np.where(want_r >= 0, want_r + spec.base, -1)
    assert np.array_equal(r1[picks], want_r), (picks, r1[picks][:, :4], want_r[:, :4])
    assert np.array_equal(s1[picks].view(np.int64), want_s.view(np.int64)), "scores differ from the C oracle"
    _sanity(s1, r1, spec.n, k, "min_score" in kw)
    if "min_score" not in kw:
        for pos, (lo, hi) in expect.items():
            assert r1[pos, :2].tolist() == [lo, hi][:k], (pos, r1[pos, :4], lo, hi)
    if thr == "above-all":
        assert (r1 == -1).all()
    if thr == "below-all":
        assert (r1[:, :min(spec.n, k)] >= 0).all()
    return r1


@pytest.mark.parametrize("case", CASES_A, ids=lambda c: c.id)
def test_few_query_cascade(case):
    run_case(case)


@pytest.mark.parametrize("case", CASES_B, ids=lambda c: c.id)
def test_emit_instantiations(case):
    run_case(case)


@pytest.mark.parametrize("case", CASES_C, ids=lambda c: c.id)
def test_gemm_class_scan(case):
    run_case(case)


@pytest.mark.parametrize("case", CASES_D, ids=lambda c: c.id)
def test_list_scan(case):
    run_case(case)


@pytest.mark.parametrize("case", CASES_E, ids=lambda c: c.id)
def test_fill_levels(case):
    run_case(case)


@pytest.mark.parametrize("case", CASES_F, ids=lambda c: c.id)
def test_ring_head(case):
    run_case(case)


@pytest.mark.parametrize("thr", G_THRESHOLDS)
@pytest.mark.parametrize("score_mode", [0, 1], ids=["raw", "unit"])
@pytest.mark.parametrize("table", sorted(G_BASE))
def test_min_score_and_score_mode(table, score_mode, thr):
    run_case(G_BASE[table], score_mode=score_mode, thr=thr)


@pytest.mark.parametrize("case", CASES_H, ids=lambda c: c.id)
def test_large_k_exhaustive(case):
    run_case(case)


# ---------------------------------------------------------------------------------------------------------------------
# I. grouped memories: fresh (0, 3, 500 groups in a 100k memory) and a 100k ring that wraps mid-group
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("D", [256, 512])
@pytest.mark.parametrize("groups", [0, 3, 500])
def test_grouped_fresh_memory(groups, D, dtype):
    from tests.search_checks import grouped_check
    from tests.support import clustered, grouped_memory, queries_near
    from vidmem.memory import EmbeddingMemory
    if groups == 0:
        mem = EmbeddingMemory(100_000, D, dtype, grouped=True)
        g = torch.Generator(device="cuda").manual_seed(D)
        q = torch.randn((16, D), generator=g, device="cuda").to(TD[dtype])
    else:
        sizes = [int(x) for x in np.random.default_rng(groups + D).integers(1, 24, groups)]
        rows, _ = clustered(sizes, D, dtype, seed=groups + D)
        mem = grouped_memory(rows, sizes, dtype, capacity=100_000)
        q = queries_near(rows, 16, 5, dtype)
    for k in (1, 10):
        r, s, kk = grouped_check(mem, q, k, dtype)
        n_groups = groups
        assert (r[:, min(n_groups, k):] == -1).all() and (s[:, min(n_groups, k):] == 0.0).all()
        assert (r[:, :min(n_groups, k)] >= 0).all()
    mem.close()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_grouped_ring_wraps_mid_group(dtype):
    from tests.search_checks import grouped_check
    from tests.support import clustered, grouped_memory, queries_near
    D, cap = 128, 100_000
    sizes = [int(x) for x in np.random.default_rng(7).integers(1, 40, 5_200)]
    while sum(sizes) <= cap + 20:
        sizes.append(13)
    rows, _ = clustered(sizes, D, dtype, seed=17)
    mem = grouped_memory(rows, sizes, dtype, capacity=cap, ring=True)
    total = sum(sizes)
    cut = total - cap                       # the oldest live row: make sure it sits inside a group
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    assert cut not in set(starts.tolist())
    grouped_check(mem, queries_near(rows[-cap:], 8, 9, dtype), 10, dtype)
    grouped_check(mem, queries_near(rows[cut - 50:cut + 50], 8, 11, dtype), 5, dtype)
    mem.close()
