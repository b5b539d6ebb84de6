"""GPU: the top-k certificate outside unit-norm rows (DESIGN.md 4.1 "Domain of the certificate", csrc/topk_common.h).

Every other top-k test searches L2-normalised rows with randn queries: the comfortable middle of fp32's range, where
"an fp32-scanned score x 1/||q|| lies within cert_eps(D) of the exact cosine" holds.  The classes of tests/domain_ref.py
leave it: large and mixed norms (inside the certificate's domain), fp16 subnormal inputs, and bf16 norms at which the
fp32 scan under- or overflows or a row's fp32 reciprocal norm is inf (outside: the library must notice and answer
through its exhaustive routes).  Every path of the row search at the smallest shape that reaches it (named by
tests/topk_plan.py, launch counts asserted), the grouped, scoped and range entries, and the norm-reading exact entries.

All assertions are bit-exact.  A case collects every assertion that fails and reports them together.
  1. with the redo: every query equals the exhaustive twin; up to 8 picked queries equal the C oracle on the stored bits
  2. row search without the redo: every UNFLAGGED query already equals the exhaustive answer (the certification claim)
  3. inside classes: nothing but the zero query is flagged (range: rescored == counts where the oracle shows a clean gap)
  4. exact classes: the answer of the unscaled memory to the unscaled queries, for all queries
"""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch

from tests import domain_ref as DR
from tests import group_ref as G
from tests import range_ref as R
from tests import scope_ref as S
from tests import support
from tests import topk_plan as TP
from tests.topk_ref import oracle_rows_parallel

pytestmark = pytest.mark.gpu

D = 256
THREADS = min(16, os.cpu_count() or 1)
SIZES = {"small": (4_099, 4_099), "large": (65_536, 65_000)}      # capacity, rows
PAIR_AT = {"small": [4_096, 2_000], "large": [4_096, 16_384, 32_768, 60_928, 64_999]}   # pass limits, dense range edges
CLASS_NAMES = list(DR.CLASSES)


def _same(a_s, a_r, b_s, b_r):
    return (a_r == b_r).all(1) & (a_s.view(np.int64) == b_s.view(np.int64)).all(1)


def _np(*ts):
    return [t.cpu().numpy() for t in ts]


def _memory(rows, dtype, cap, **kw):
    from vidmem.memory import EmbeddingMemory
    mem = EmbeddingMemory(cap, rows.shape[1], dtype, **kw)
    for lo in range(0, rows.shape[0], 20_011):
        mem.append(rows[lo:lo + 20_011])
    return mem


@functools.lru_cache(maxsize=None)
def dataset(name, size):
    """The class's data at one size and its memory, shared by the cases that search it."""
    cap, n = SIZES[size]
    ds = DR.domain_set(name, n, D, seed=11, device="cuda", pair_at=PAIR_AT[size])
    assert ds.rows_exact == ds.cls.exact or ds.cls.rnorm_plants, "the class's exactness precondition"
    return ds, _memory(ds.rows, ds.cls.dtype, cap), DR.bits(ds.rows)


@functools.lru_cache(maxsize=None)
def unscaled_answer(dtype, size, Q, k):
    """Exhaustive top-k of the UNSCALED rows for the unscaled queries: the base rows and queries depend on the dtype and
    the seeds only, so every class of one dtype shares it."""
    name = next(c.name for c in DR.CLASSES.values() if c.dtype == dtype and c.exact)
    ds = DR.domain_set(name, SIZES[size][1], D, seed=11, device="cuda", pair_at=PAIR_AT[size])
    qb = ds.queries(Q, seed=Q * 7919 + k)[0]
    mem = _memory(ds.base, dtype, SIZES[size][0])
    s, r = _np(*mem.topk(qb, k, exact=True))
    mem.close()
    return s, r


def _gscan_q(cap):
    """The smallest Q from 2,048 up whose two passes over a 65,536-row memory are both GEMM-class on this device."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    Q = 2_048
    while Q < 16_384:
        p = TP.plan(Q, 10, D, "f16", cap, cus)
        if p.family == "cascade" and all(x.kind == "gscan" for x in p.passes[1:]):
            return Q
        Q += 256
    raise AssertionError("no Q reaches the GEMM-class scan on this device")


# path, size, Q (None: computed from the device), k, family, what the mirror must say
ROW_CASES = [("list-QT1", "small", 5, 5, "list"), ("list-QT2", "small", 33, 12, "list"),
             ("prepass", "large", 33, 10, "list+prepass"), ("emit-NG1", "large", 64, 10, "cascade"),
             ("emit-NG2", "large", 200, 10, "cascade"), ("gscan", "large", None, 10, "cascade")]


@pytest.mark.parametrize("case", ROW_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("name", CLASS_NAMES)
def test_row_search(name, case):
    from vidmem.memory import TopkScratch
    path, size, Q, k, family = case
    cap, n = SIZES[size]
    cls = DR.CLASSES[name]
    if Q is None:
        Q = _gscan_q(cap)
    plan = TP.plan(Q, k, D, cls.dtype, cap, torch.cuda.get_device_properties(0).multi_processor_count)
    assert plan.family == family, (plan.family, family)
    if path.startswith("list"):
        assert plan.QT == int(path[-1])
    elif path.startswith("emit"):
        assert plan.NG == int(path[-1]) and all(x.kind == "emit" for x in plan.passes[1:])
    elif path == "gscan":
        assert all(x.kind == "gscan" for x in plan.passes[1:]) and len(plan.passes) == 3
    ds, mem, live = dataset(name, size)
    qb, qs, q_exact, picks, zero = ds.queries(Q, seed=Q * 7919 + k)
    assert q_exact == cls.exact or cls.rnorm_plants
    es, er = _np(*mem.topk(qs, k, exact=True))
    scratch = TopkScratch.for_(mem, Q, k)
    (s0, r0), launches = support.launches(mem, lambda: mem.topk(qs, k, redo=False, scratch=scratch), ("topk_scan", "topk_finalize"))
    assert launches == plan.launches, (path, launches, plan.launches)
    flags = scratch.flags[:Q].cpu().numpy()
    s0, r0 = _np(s0, r0)
    problems = []
    bad = np.flatnonzero((flags == 0) & ~_same(s0, r0, es, er))
    if bad.size:
        problems.append(f"2. {bad.size} certified (unflagged) queries differ from the exhaustive answer: {bad[:6].tolist()}")
    flagged = set(np.flatnonzero(flags).tolist())
    if cls.inside and not flagged <= {zero}:
        problems.append(f"3. inside the domain, yet flagged: {sorted(flagged)[:6]} (zero query {zero})")
    scratch.uncert.zero_()
    s1, r1 = _np(*mem.topk(qs, k, scratch=scratch))
    bad = np.flatnonzero(~_same(s1, r1, es, er))
    if bad.size:
        problems.append(f"1. {bad.size} queries differ from the exhaustive answer after the redo: {bad[:6].tolist()}")
    want_r, want_s = oracle_rows_parallel(DR.bits(qs), live, k, cls.dtype, picks, threads=THREADS)
    if not _same(s1[picks], r1[picks], want_s, want_r).all():
        problems.append(f"1. picked queries differ from the C oracle: {np.asarray(picks)[~_same(s1[picks], r1[picks], want_s, want_r)]}")
    if not _same(es[picks], er[picks], want_s, want_r).all():
        problems.append("1. the exhaustive kernel differs from the C oracle")
    if cls.exact:
        us, ur = unscaled_answer(cls.dtype, size, Q, k)
        bad = np.flatnonzero(~_same(s1, r1, us, ur))
        if bad.size:
            problems.append(f"4. {bad.size} queries differ from the unscaled memory's answer: {bad[:6].tolist()}")
    print(f"[domain] {name} {path} Q={Q}: flagged {len(flagged)} of {Q}" + "".join("\n    " + p for p in problems))
    assert not problems, problems


# ---- grouped, scoped, range: n = 4,099 ------------------------------------------------------------------------------
def _grouped(rows, dtype):
    from tests.support import grouped_memory
    sizes = [5] * 819 + [4]
    return grouped_memory(rows, sizes, dtype)


@pytest.mark.parametrize("name", CLASS_NAMES)
def test_grouped(name):
    Q, k = 16, 10
    cls = DR.CLASSES[name]
    ds, _, live = dataset(name, "small")
    qb, qs, _, picks, zero = ds.queries(Q, seed=77)
    mem = _grouped(ds.rows, cls.dtype)
    s1, r1, k1 = _np(*mem.topk_grouped(qs, k))
    flags = mem.last_group_flags[:Q].cpu().numpy()
    es, er, ek = _np(*mem.topk_grouped(qs, k, exact=True))
    keys = mem.group_keys_host()
    problems = []
    bad = np.flatnonzero(~(_same(s1, r1, es, er) & (k1 == ek).all(1)))
    if bad.size:
        problems.append(f"1. {bad.size} queries differ from the exhaustive entry: {bad[:6].tolist()}")
    want_r, want_s, want_k = G.grouped_topk(DR.bits(qs)[picks], live, keys, k, dtype=cls.dtype)
    if not (_same(s1[picks], r1[picks], want_s, want_r).all() and np.array_equal(k1[picks], want_k)):
        problems.append("1. picked queries differ from the oracle")
    flagged = set(np.flatnonzero(flags).tolist())
    if cls.inside and not flagged <= {zero}:
        problems.append(f"3. inside the domain, yet flagged: {sorted(flagged)} (zero query {zero})")
    if cls.exact:
        base = _grouped(ds.base, cls.dtype)
        us, ur, uk = _np(*base.topk_grouped(qb, k, exact=True))
        base.close()
        if not (_same(s1, r1, us, ur).all() and np.array_equal(k1, uk)):
            problems.append("4. differs from the unscaled memory's answer")
    mem.close()
    print(f"[domain] {name} grouped: flagged {len(flagged)} of {Q}" + "".join("\n    " + p for p in problems))
    assert not problems, problems


@pytest.mark.parametrize("name", CLASS_NAMES)
def test_scoped(name):
    from tests.support import contiguous_tags, mixed_scopes, tagged_memory
    Q, k = 16, 10
    cls = DR.CLASSES[name]
    ds, _, live = dataset(name, "small")
    qb, qs, _, picks, zero = ds.queries(Q, seed=78)
    tags = contiguous_tags(ds.n, 8)
    scopes = mixed_scopes(tags, Q, k)
    mem = tagged_memory(ds.rows, tags, cls.dtype)
    s1, r1 = _np(*mem.topk_scoped(qs, k, scopes))
    flags = mem.last_scope_flags[:Q].cpu().numpy()
    es, er = _np(*mem.topk_scoped(qs, k, scopes, exact=True))
    problems = []
    bad = np.flatnonzero(~_same(s1, r1, es, er))
    if bad.size:
        problems.append(f"1. {bad.size} queries differ from the exhaustive entry: {bad[:6].tolist()}")
    want_r, want_s = S.scoped_topk(DR.bits(qs)[picks], live, tags, [scopes[i] for i in picks], k, dtype=cls.dtype)
    if not _same(s1[picks], r1[picks], want_s, want_r).all():
        problems.append("1. picked queries differ from the oracle")
    flagged = set(np.flatnonzero(flags).tolist())
    if cls.inside and not flagged <= {zero}:
        problems.append(f"3. inside the domain, yet flagged: {sorted(flagged)} (zero query {zero})")
    if cls.exact:
        base = tagged_memory(ds.base, tags, cls.dtype)
        us, ur = _np(*base.topk_scoped(qb, k, scopes, exact=True))
        base.close()
        if not _same(s1, r1, us, ur).all():
            problems.append("4. differs from the unscaled memory's answer")
    mem.close()
    print(f"[domain] {name} scoped: flagged {len(flagged)} of {Q}" + "".join("\n    " + p for p in problems))
    assert not problems, problems


@pytest.mark.parametrize("name", CLASS_NAMES)
def test_range(name):
    from tests.support import clustered
    from tests.search_checks import range_memory, raw_range
    Q = 17
    cls = DR.CLASSES[name]
    rows, _ = clustered([5] * 819 + [4], D, cls.dtype, seed=5)
    ds = DR.domain_set(name, 4_099, D, seed=12, device="cuda", pair_at=[], base=rows)
    assert ds.rows_exact == cls.exact or cls.rnorm_plants
    qb, qs, q_exact, _, zero = ds.queries(Q, seed=79, near=True)
    assert q_exact == cls.exact or cls.rnorm_plants
    mem = range_memory(ds.rows, cls.dtype)
    matrix = R.cref.cosine_matrix(DR.bits(qs), DR.bits(ds.rows), dtype=cls.dtype)
    problems = []
    for tau in (0.2, -1.0):
        want = R.range_from_scores(matrix, tau)
        width = max(c for _, _, c in want) + 3 if tau == 0.2 else 100
        want_r, want_s, want_c = R.padded(want, width)
        got = {}
        for exact in (False, True):
            rc, r, s, c, resc = raw_range(mem, qs, tau, max_hits=width, exact=exact)
            assert rc == 0, (rc, mem.L.vm_last_error(mem.ctx.handle))
            got[exact] = (r, s, c)
            ok = np.array_equal(c, want_c) and np.array_equal(r, want_r) and np.array_equal(s.view(np.int64), want_s.view(np.int64))
            if not ok:
                problems.append(f"1. tau={tau} {'exhaustive' if exact else 'fast'} entry differs from the oracle: "
                                f"counts {c[:6].tolist()} want {want_c[:6].tolist()}")
            if not exact:
                if not (resc >= c).all():
                    problems.append(f"tau={tau}: fewer pairs re-scored than hits")
                if cls.inside:     # precondition from the oracle, per query: no exact score within 4 eps of the threshold
                    clean = np.abs(matrix - tau).min(1) > 4 * R.cert_eps(D)
                    assert clean.sum() >= Q // 2, "precondition: most queries have a clean gap at the threshold"
                    if not np.array_equal(resc[clean], c[clean]):
                        problems.append(f"3. tau={tau}: re-scored {resc[clean][:6].tolist()} != hits {c[clean][:6].tolist()} "
                                        f"on queries with a clean gap")
        if tau == -1.0 and cls.inside:
            assert (want_c == ds.n).all()
        if cls.exact:
            base = range_memory(ds.base, cls.dtype)
            rc, ur, us, uc, _ = raw_range(base, qb, tau, max_hits=width, exact=True)
            base.close()
            r, s, c = got[False]
            if not (rc == 0 and np.array_equal(c, uc) and np.array_equal(r, ur) and np.array_equal(s.view(np.int64), us.view(np.int64))):
                problems.append(f"4. tau={tau}: differs from the unscaled memory's answer")
    mem.close()
    print(f"[domain] {name} range" + "".join("\n    " + p for p in problems))
    assert not problems, problems


# ---- the norm-reading exact entries ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bf16_mixed", "bf16_under", "bf16_over"])
def test_events_links_and_novelty_append_read_the_scaled_norms(name):
    """vm_memory_events' links and vm_memory_append_novel's keep / row_of on a 1,025-row memory: exact-only code, but it
    reads the stored norms (and the novelty append searches the memory first): bit-identical to the unscaled run."""
    from tests import events_ref as E
    cls = DR.CLASSES[name]
    n, B = 1_025, 48
    ds = DR.domain_set(name, n, D, seed=21, device="cuda", pair_at=[200, 201 + 2, 700])
    assert ds.rows_exact
    g = torch.Generator(device="cuda").manual_seed(5)
    batch = torch.randn((B, D), generator=g, device="cuda")
    src = torch.randint(0, n, (B // 2,), generator=g, device="cuda")
    batch[::2] = ds.base[src].float() + 0.02 * batch[::2]          # every other row resembles a stored one
    batch[5] = batch[3]                                            # and one resembles an earlier row of the batch
    bb = DR._unit16(batch, cls.dtype)
    lo, hi = cls.row_exp
    bs, exact = DR.scaled(bb, torch.randint(lo, hi + 1, (B,), generator=g, device="cuda", dtype=torch.int32))
    assert exact
    out = []
    for rows, new in ((ds.base, bb), (ds.rows, bs)):
        mem = _memory(rows, cls.dtype, n + B)
        ev = mem.events(0.5, with_links=True)
        nov = mem.append_novel(new, 0.8)
        out.append((ev.links.cpu().numpy(), ev.first_rows.cpu().numpy(), ev.count, nov.keep.cpu().numpy(),
                    nov.row_of.cpu().numpy(), nov.kept))
        mem.close()
    a, b = out
    want_links = E.links(DR.bits(ds.rows), cls.dtype)
    assert np.array_equal(b[0][1:].view(np.int64), np.asarray(want_links, np.float64)[1:].view(np.int64)), "links differ from the oracle"
    assert np.array_equal(a[0][1:].view(np.int64), b[0][1:].view(np.int64)), "links differ from the unscaled run"
    assert np.array_equal(a[1], b[1]) and a[2] == b[2] and 1 < a[2] < n
    assert np.array_equal(a[3], b[3]), ("keep differs from the unscaled run", np.flatnonzero(a[3] != b[3])[:8])
    assert np.array_equal(a[4], b[4]), "row_of differs from the unscaled run"
    assert a[5] == b[5] and B // 2 - 2 <= a[5] < B
