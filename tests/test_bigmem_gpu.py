"""GPU: every memory operation on rows stored past 2 GiB and past 4 GiB (DESIGN.md "Rows past 4 GiB").

One fp16 memory of 2^21 + 70,003 rows x 1,024 dims (4.44 GB; row 2^20 lies at byte offset 2^31, row 2^21 at byte offset 2^32
and element offset 2^31), grouped and tagged, built on the device in 65,536-row blocks of noise with planted rows around
both boundaries, at a control site below 2 GiB, at rows 0 - 1 and at the tail (tests/bigmem_ref.py).  Every expectation is
the search's own oracle over the neighbourhoods of those sites, which the helper proves sufficient from the oracle's
numbers alone (tests/test_bigmem_cpu.py: equal to the dense oracle on a small layout).  Rows equal, fp64 scores bit-equal;
where the oracle's gap condition holds the fast path must certify the query itself (flag 0): a wrong scan may not hide
behind the redo.  No tolerance anywhere.

The biased, the any/all and the sequence search run on the same memory (``test_biased``, ``test_fold``, ``test_seq``, and once
more each behind the erase and in the ring; one biased call in bf16): the two bias columns as ``bias_of_rows`` and
``bias_of_age`` build them must equal their restatements bit for bit at the sites, the fold's term indices and the
sequences' step rows and step score bits must be the oracle's.  ``test_biased`` and ``test_fold`` demand flag 0 of all 16
queries (the model asserts ``bias_ref.flag0_ok`` / ``fold_ref.flag0_ok`` for each); ``test_seq`` demands it wherever
``seq_ref.margin``'s condition holds over the merged runs above 4 eps_seq - of every sequence at k = 1 (asserted) - and
prints how many sequences were flagged and how many had to be certified.

Read-only tests first, then the gated append, the erase and the ring; the mutating tests update the model, so every test
derives its expectation from the model as it is.  One memory at a time: the ring test closes the first one.
With BIGMEM_JSON set, the wall time of the build and of every test and the device memory the fixture took are written to
that file (the tests assert, the file only reports).
"""
from __future__ import annotations

import json
import os
import time

import numpy as np
import pytest
import torch

from tests import bigmem_ref as B
from tests import diverse_ref as DR
from tests import novelty_ref as NV
from tests import support
from tests import topk_plan as TP
from tests.support import bits, from_bits, np_of

pytestmark = pytest.mark.gpu

L = B.BIG
CAP = L.N + L.spare
REPORT = {"layout": L._asdict(), "bytes_of_rows": L.N * L.D * 2, "tests": {}}


def _pair(got_s, got_r, want, what):
    """(scores, rows) of the memory against (rows, scores) of the oracle."""
    r, s = np_of(got_r), np.ascontiguousarray(np_of(got_s), np.float64)
    assert np.array_equal(r, want[0]), f"{what} rows: first difference at query {int(np.argmax((r != want[0]).any(1)))}: " \
                                       f"{r[(r != want[0]).any(1)][:2].tolist()} != {want[0][(r != want[0]).any(1)][:2].tolist()}"
    assert np.array_equal(s.view(np.int64), np.ascontiguousarray(want[1]).view(np.int64)), what + " scores (bit-exact bar)"


def _flags0(flags, Q, what):
    f = np_of(flags)[:Q]
    assert not f.any(), f"{what}: the fast path left queries {np.flatnonzero(f).tolist()[:8]} to the redo, flags {f[f != 0][:8]}"


def _build(ring: bool, dtype="f16"):
    from vidmem.memory import EmbeddingMemory
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    t0 = time.perf_counter()
    total = L.N + 300 if ring else L.N
    mem = EmbeddingMemory(L.N if ring else CAP, L.D, dtype, ring=ring, grouped=True, tagged=True)
    gen = torch.Generator(device="cuda").manual_seed(2024)
    cand = {}
    for start, x, keys, tags in B.blocks(L, gen, "cuda", total=total, dtype=dtype):
        B.cut_hoods(L, start, x, cand)
        assert mem.append(x, group=keys, tag=tags) == start
    del x, keys, tags
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    torch.cuda.empty_cache()
    used = free0 - torch.cuda.mem_get_info()[0]
    model = B.Sparse(L, cand, total=total, dtype=dtype)
    if ring:
        model.drop_below(total - L.N)
    assert len(mem) == total
    return mem, model, seconds, used


class State:
    """The memory under test and its model; the ring test swaps both."""
    mem = None
    model = None


@pytest.fixture(scope="module")
def st():
    s = State()
    s.mem, s.model, REPORT["build_seconds"], REPORT["device_bytes_taken"] = _build(ring=False)
    yield s
    if s.mem is not None:
        s.mem.close()
    s.mem = None
    torch.cuda.empty_cache()
    path = os.environ.get("BIGMEM_JSON")
    if path:
        REPORT["device"] = torch.cuda.get_device_name(0)
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


@pytest.fixture(autouse=True)
def _timed(request):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    REPORT["tests"][request.node.name] = round(time.perf_counter() - t0, 3)


def _gather(mem, column, rows):
    """A per-slot column of the memory at the slots of ``rows``, indexed on the device."""
    from vidmem.memory import _tensor_from_ptr
    ptr = mem.L.vm_memory_group_keys(mem.handle) if column == "keys" else mem.L.vm_memory_tags(mem.handle)
    col = _tensor_from_ptr(ptr, (mem.searchable,), torch.int64, mem.device)
    return col[torch.from_numpy(np.asarray(rows, np.int64) % mem.capacity).cuda()].cpu().numpy()


def _read_back(mem, model, what):
    slots = torch.from_numpy(model.gid % mem.capacity).cuda()
    assert np.array_equal(bits(mem.rows_tensor()[slots]), model.rows), what + ": rows_tensor differs at the sites"
    assert np.array_equal(_gather(mem, "keys", model.gid), model.keys), what + ": group keys differ at the sites"
    assert np.array_equal(_gather(mem, "tags", model.gid), model.tags), what + ": tags differ at the sites"


# ---- read only -----------------------------------------------------------------------------------------------------------
def test_append_read_back(st):
    mem, model = st.mem, st.model
    assert mem.rows_tensor().shape == (L.N, L.D) and mem.rows_tensor().numel() > 1 << 31
    _read_back(mem, model, "append")
    for b in (L.b1, L.b2):      # planted bits on both sides of each boundary
        plant = B.planted_rows(L)
        for r in (b - 1, b):
            assert np.array_equal(bits(mem.rows_tensor()[r]), plant[r]), r


# Q -> (family, kinds of the cascade's passes after the dense one).  256 x 256 tiles: 160 queries have enough of them only
# in the pass over [262,144, 2^21), which crosses 2 GiB; 800 queries also in the last pass, which begins at 4 GiB.
PLAIN = {4: ("list", ""), 20: ("list+prepass", ""), 60: ("cascade", "ee"), 160: ("cascade", "eege"), 800: ("cascade", "eggg")}


def _plain(mem, model, Q, what=""):
    from vidmem.memory import TopkScratch
    dtype = model.dtype
    q = B.queries(L, Q, Q, dtype=dtype)
    want = model.topk(q, B.K)
    plan = TP.plan(Q, B.K, L.D, dtype, mem.capacity, torch.cuda.get_device_properties(0).multi_processor_count)
    kinds = "".join("g" if p.kind == "gscan" else "e" for p in plan.passes[1:])
    assert (plan.family, kinds) == PLAIN[Q], (plan.family, kinds)
    if Q >= 160:        # the last pass begins exactly at byte offset 2^32
        assert (plan.passes[-1].begin, plan.passes[-1].limit) == (L.b2, None), plan.passes
    scratch = TopkScratch.for_(mem, Q, B.K)
    (s, r), launches = support.launches(mem, lambda: mem.topk(from_bits(q, dtype), B.K, redo=False, scratch=scratch))
    assert (launches["topk_scan"], launches["topk_finalize"]) == (plan.launches["topk_scan"], plan.launches["topk_finalize"]), \
        (plan.family, launches, plan.launches)
    _flags0(scratch.flags, Q, f"{what}topk Q={Q} redo=False")
    _pair(s, r, want, f"{what}topk Q={Q} redo=False")
    mem.reset_uncertified()
    s, r = mem.topk(from_bits(q, dtype), B.K)
    _pair(s, r, want, f"{what}topk Q={Q}")
    _flags0(mem._last[TopkScratch].flags, Q, f"{what}topk Q={Q}")
    assert mem.uncertified_count == 0
    return want


@pytest.mark.parametrize("Q", sorted(PLAIN))
def test_topk(st, Q):
    want = _plain(st.mem, st.model, Q)
    rows = want[0]                          # the answers lie on both sides of both boundaries
    assert (rows >= L.b2).any() and (rows < L.b1).any() and ((rows >= L.b1) & (rows < L.b2)).any()


def test_topk_exact_and_exhaustive(st):
    mem, model = st.mem, st.model
    q = B.queries(L, 4, 4)
    s, r = mem.topk(from_bits(q), B.K, exact=True)
    _pair(s, r, model.topk(q, B.K), "topk exact")
    (s, r), launches = support.launches(mem, lambda: mem.topk(from_bits(q), 59, min_score=B.RANGE_MIN))
    assert launches["topk_scan"] == 0 and launches["topk_exact"] >= 1, launches
    want = model.topk(q, 59, min_score=B.RANGE_MIN)
    assert ((want[0] >= 0).sum(1) == [B.LEVELS + 1, B.LEVELS + 1, B.LEVELS, B.LEVELS]).all()
    _pair(s, r, want, "topk k=59")


def _both(call, want, flags, Q, what, keys=None, third="keys"):
    """One filtered search in its fast and its exact form; ``flags``: a callable -> the fast call's flags.  ``keys``: what
    the call's third output must be, named ``third`` in the failure."""
    for exact in (False, True):
        out = call(exact)
        form = what + (" exact" if exact else "")
        _pair(out[0], out[1], want, form)
        if keys is not None:
            assert np.array_equal(np_of(out[2]), keys), f"{form} {third}"
        if not exact:
            _flags0(flags(), Q, form)


def _scoped_and_grouped(mem, model, what=""):
    q = B.queries(L, 16, 7)
    tq = from_bits(q)
    want = model.grouped(q, B.K)
    _both(lambda e: mem.topk_grouped(tq, B.K, exact=e), want, lambda: mem.last_group_flags, 16, what + "grouped", want[2])
    for name, (scope, k, gk) in B.scope_cases(L).items():
        _both(lambda e: mem.topk_scoped(tq, k, scope, exact=e), model.scoped(q, scope, k), lambda: mem.last_scope_flags, 16,
              f"{what}scoped {name}")
        want = model.grouped_scoped(q, scope, gk)
        _both(lambda e: mem.topk_grouped_scoped(tq, gk, scope, exact=e), want, lambda: mem.last_group_scope_flags, 16,
              f"{what}grouped scoped {name}", want[2])


def test_scoped_and_grouped(st):
    _scoped_and_grouped(st.mem, st.model)
    got = st.model.grouped(B.queries(L, 16, 7), B.K)[0]
    for f in range(B.FAMILIES):     # levels 0 and 6 share a group above b2: only the better one is returned
        m = B.members(L, f)
        assert m[0] in got[f] and m[6] not in got[f]


def test_masked(st):
    mem, model = st.mem, st.model
    q = B.queries(L, 16, 8)
    ids = B.mask_rows(L)
    mask = mem.mask_of_rows(ids)
    _both(lambda e: mem.topk_masked(from_bits(q), B.K, mask, exact=e), model.masked(q, model.sel_of_rows(ids, 16), B.K),
          lambda: mem.last_mask_flags, 16, "masked mask_of_rows")
    scope, k, _ = B.scope_cases(L)["sources above b2"]
    mask = mem.mask_of_scope(scope)
    assert not bool(mask[:L.b2 // 32].any()) and bool(mask[L.b2 // 32:].any())      # no bit below row 2^21
    _both(lambda e: mem.topk_masked(from_bits(q), k, mask, exact=e), model.masked(q, model.sel_of_scope(scope, 16), k),
          lambda: mem.last_mask_flags, 16, "masked mask_of_scope")


def _spans(mem, model, what=""):
    q = B.queries(L, 16, 8)
    for name, (fam, spans, k) in B.span_cases(L).items():
        qq = q[list(fam)]
        _both(lambda e: mem.topk_span(from_bits(qq), k, spans, exact=e), model.span(qq, spans, k), lambda: mem.last_span_flags,
              len(fam), f"{what}span {name}")


def test_span(st):
    _spans(st.mem, st.model)


def _range(mem, model, what=""):
    q = B.queries(L, 16, 9)
    scope = B.scope_cases(L)["sources above b2"][0]
    for sc in (None, [scope] * 16):
        want = model.range(q, B.RANGE_MIN, sc)
        for exact in (False, True):
            hits = mem.range_search(from_bits(q), B.RANGE_MIN, scope=sc, max_hits=64, exact=exact)
            for f, (h, w) in enumerate(zip(hits, want)):
                form = f"{what}range {'scoped ' if sc else ''}{'exact ' if exact else ''}query {f}"
                assert h.count == w[2] <= 64, f"{form}: {h.count} hits, want {w[2]}"       # never truncated
                _pair(h.scores[None], h.rows[None], (w[0][None], w[1][None]), form)
    return want


def test_range(st):
    _range(st.mem, st.model)
    want = st.model.range(B.queries(L, 16, 9), B.RANGE_MIN)
    for f, w in enumerate(want):       # exactly the family's members, in time order
        assert w[0].tolist() == sorted(B.members(L, f).values())


def _clip(mem, model, clips, k, min_sep, gap, min_score, what):
    """One clip search, fast and exact; where the oracle's margin condition holds the fast path must certify the clip."""
    want = model.clip(clips, k, min_sep, min_score, max_gap_ms=-1 if gap is None else gap)
    for exact in (False, True):
        s, r = mem.topk_clip(from_bits(clips), k, min_sep=min_sep, max_gap_ms=gap, min_score=min_score, exact=exact)
        _pair(s, r, want, what + (" exact" if exact else ""))
        if not exact:
            flags = np_of(mem.last_clip_flags)[:clips.shape[0]]
            bad = np.flatnonzero(want[2] & (flags != 0))
            assert bad.size == 0, f"{what}: the fast path left clips {bad.tolist()} to the redo, flags {flags.tolist()}"
    return want


@pytest.mark.parametrize("min_sep", [1, 4])
@pytest.mark.parametrize("gap", [None, 1])
def test_clip(st, min_sep, gap):
    mem, model = st.mem, st.model
    clips = B.clips_of(L)
    starts, cut = B.clip_cases(L)
    # k = 1: every clip meets clip_ref.margin's condition, so every clip is answered by the fast path itself
    want = _clip(mem, model, clips, 1, min_sep, gap, None, f"clip k=1 min_sep={min_sep} max_gap_ms={gap}")
    assert want[2].all(), want[2]
    for c, (s0, broken) in enumerate(zip(starts, cut)):     # the windows across the source changes at b1, b2 are no windows
        assert (want[0][c, 0] != s0) if broken else want[0][c, 0] == s0, (c, want[0][c])
    # k = 3 above min_score: the later peaks are partial matches (windows of the same families elsewhere) below the
    # filter; the helper's condition decides per clip whether the fast path must certify it
    want = _clip(mem, model, clips, B.CLIP_K, min_sep, gap, B.CLIP_MIN, f"clip k=3 min_sep={min_sep} max_gap_ms={gap}")
    for c, (s0, broken) in enumerate(zip(starts, cut)):
        assert (s0 not in want[0][c]) if broken else want[0][c, 0] == s0, (c, want[0][c])


def test_mix(st):
    mem, model = st.mem, st.model
    terms, w = B.mix_terms(L), [B.MIX_W] * 16
    _both(lambda e: mem.topk_mix(from_bits(terms), w, B.MIX_K, exact=e), model.mix(terms, w, B.MIX_K), lambda: mem.last_mix_flags,
          16, "mix")


def test_diverse(st):
    mem, model = st.mem, st.model
    q, lam = B.queries(L, 16, 10), DR.lam_vector(16)
    want = model.diverse(q, B.DIV_K, B.POOL, lam)
    for exact in (False, True):
        s, r = mem.topk_diverse(from_bits(q), B.DIV_K, pool=B.POOL, lam=lam, exact=exact)
        _pair(s, r, want, "diverse" + (" exact" if exact else ""))
        assert np.array_equal(np_of(mem.last_diverse_mmr).view(np.int64), want[2].view(np.int64)), "diverse mmr"
        if not exact:
            _flags0(mem.last_diverse_flags, 16, "diverse")
    picked = want[0]
    assert (picked >= L.b2).any(1).all() and (picked < L.b2).any(1).all()      # picks from both sides of 4 GiB


def test_summaries(st):
    mem, model = st.mem, st.model
    groups = int(model.keys[-1]) + 1
    ref = model.summaries()
    for g0 in (L.b2 // B.GROUP - 2, groups - 4):
        sm = mem.summaries(first_group=g0, max_groups=4)
        assert sm.count == groups
        at = np.searchsorted(ref.keys, np.arange(g0, g0 + 4))
        assert np.array_equal(ref.keys[at], np.arange(g0, g0 + 4))          # whole groups of the neighbourhoods
        for name in ("first_rows", "n_rows", "keys", "key_rows"):
            assert np.array_equal(np_of(getattr(sm, name)), getattr(ref, name)[at]), f"summaries at group {g0}: {name}"
        assert np.array_equal(bits(sm.centroids), ref.centroids[at]), f"summaries at group {g0}: centroids"
        assert np.array_equal(np_of(sm.key_scores).view(np.int64), ref.key_scores[at].view(np.int64)), "summaries key_scores"


def test_events(st):
    mem, model = st.mem, st.model
    n = model.total
    inner = np.zeros(n, bool)           # rows whose link to the row before lies inside one neighbourhood
    for lo, hi in model.inner():
        inner[lo:hi] = True
    # independent of the library: no other adjacent pair resembles each other, so each such row opens an event
    rows = mem.rows_tensor()
    worst = 0.0
    for s in range(1, n, L.block):
        e = min(n, s + L.block)
        x = rows[s - 1:e].float()
        x = x / x.norm(dim=1, keepdim=True)
        cos = (x[1:] * x[:-1]).sum(1)
        cos[torch.from_numpy(inner[s:e]).cuda()] = 0.0
        worst = max(worst, float(cos.max()))
    assert worst < 0.4, worst
    count, event_of, first, closed = model.events(0.5, 0.4)
    assert closed.size == B.FAMILIES                   # levels 0 and 6 of each family, side by side above b2
    ev = mem.events(0.5)
    assert ev.count == count
    got = ev.event_of[torch.from_numpy(model.gid).cuda()].cpu().numpy()
    assert np.array_equal(got, event_of), "event_of at the sites"
    assert np.array_equal(ev.first_rows[torch.from_numpy(event_of).cuda()].cpu().numpy(), first), "first_rows at the sites"


# ---- the three newer searches: biased, any/all, sequence -------------------------------------------------------------------
def _bias_columns(mem, model, what=""):
    """The two columns as the device builds them -> (device fp32 [2, S], the model's columns).  At the sites each must be
    the builder's restatement bit for bit (read by slot: ``model.gid % capacity``)."""
    rows, values = B.boost_rows(L)
    now, per_ms = model.newest_ms, B.age_per_ms(L)
    want = [model.col_of_rows(rows, values, mem.capacity), model.col_of_age(now, per_ms, B.AGE_FILL, mem.capacity)]
    cols = mem.new_bias(2)
    mem.bias_of_rows(torch.tensor(rows, dtype=torch.int64).cuda(), values, out=cols[0])
    mem.bias_of_age(now, per_ms, fill=B.AGE_FILL, out=cols[1])
    slots = torch.from_numpy(model.gid % mem.capacity).cuda()
    for name, col, w in zip(("bias_of_rows", "bias_of_age"), cols, want):
        got = col[slots].cpu().numpy()
        assert np.array_equal(got.view(np.uint32), w.at.view(np.uint32)), f"{what}{name}: the column differs at the sites"
    if mem.searchable < mem.capacity:       # slots without a live row hold the fill
        assert bool((cols[1][mem.searchable:mem.capacity] == B.AGE_FILL).all()), what + "bias_of_age: fill"
    return cols, want


def _biased(mem, model, what=""):
    dtype = model.dtype
    q, betas, index = B.queries(L, 16, 13, dtype=dtype), B.bias_weights(), list(B.BIAS_INDEX)
    cols, at = _bias_columns(mem, model, what)
    want = model.biased(q, at, index, betas, B.BIAS_K)
    _both(lambda e: mem.topk_biased(from_bits(q, dtype), B.BIAS_K, cols, weight=betas, bias_index=index, exact=e), want,
          lambda: mem.last_bias_flags, 16, what + "biased")
    return want


def test_biased(st):
    want = _biased(st.mem, st.model)
    rows = want[0]
    assert (rows >= L.b2).any() and (rows < L.b1).any() and ((rows >= L.b1) & (rows < L.b2)).any()
    for f, (c, beta) in enumerate(zip(B.BIAS_INDEX, B.bias_weights())):
        m = B.members(L, f)
        if c == 0 and beta == 1.0:          # the boosted member below 4 GiB outranks the better one above it
            assert rows[f, 0] == m[4] and m[0] in rows[f]
        if c == 1 and beta == 1.0:          # age: the member at the tail, past 4 GiB, passes the one below 2 GiB
            assert rows[f].tolist().index(m[2]) < rows[f].tolist().index(m[1])


def _fold(mem, model, op, what=""):
    terms, w = B.fold_cases(L)[op]
    want = model.fold(terms, w, B.FOLD_K, op)
    _both(lambda e: mem.topk_fold(from_bits(terms), B.FOLD_K, op=op, weights=w, exact=e), want, lambda: mem.last_fold_flags, 16,
          f"{what}fold {op}", want[2], third="term indices")
    return want


@pytest.mark.parametrize("op", ["max", "min"])
def test_fold(st, op):
    rows = _fold(st.mem, st.model, op)[0]
    assert (rows >= L.b2).any(1).all() and (rows < L.b1).any(1).all()      # every query: rows on both sides of both boundaries


def _seq(mem, model, group, k, min_score, what, G=B.SEQ_G, first=None, without=()):
    """One group of tests/bigmem_ref.seq_cases (``first``: only that many of them), fast and exact: end rows, score bits,
    step rows and step score bits; where the model's margin condition holds the fast path must certify the sequence.
    ``without``: rows no sequence may use (``~mask_of_rows``), beside the row a case excludes itself."""
    cases = B.seq_cases(L)[group][:first]
    steps = B.seq_steps(L, cases)
    sel = B.seq_sel(model, cases) & ~np.isin(model.gid, list(without))
    masks, index = None, None
    if without or any(x is not None for _, _, _, x in cases):
        sets = sorted({x for _, _, _, x in cases}, key=lambda x: -1 if x is None else x)
        drop = [list(without) + ([] if x is None else [x]) for x in sets]
        masks = torch.stack([~mem.mask_of_rows(d) if d else ~mem.new_mask()[0] for d in drop])
        index = [sets.index(x) for _, _, _, x in cases]
    want = model.seq(steps, k, G, B.SEQ_SEP, sel=sel, min_score=min_score)
    for exact in (False, True):
        s, r, sr, ss = mem.topk_seq(from_bits(steps), k, max_step=G, min_sep=B.SEQ_SEP, mask=masks, mask_index=index,
                                    min_score=min_score, exact=exact)
        form = what + (" exact" if exact else "")
        _pair(s, r, want, form)
        assert np.array_equal(np_of(sr), want[2]), form + " step rows"
        assert np.array_equal(np.ascontiguousarray(np_of(ss), np.float64).view(np.int64), want[3].view(np.int64)), form + " step scores"
        if not exact:
            flags = np_of(mem.last_seq_flags)[:len(cases)]
            bad = np.flatnonzero(want[4] & (flags != 0))
            print(f"{form}: flagged={int((flags != 0).sum())} must={int(want[4].sum())} of {len(cases)}")
            assert bad.size == 0, f"{form}: the fast path left sequences {bad.tolist()} to the redo, flags {flags.tolist()}"
    return cases, want


@pytest.mark.parametrize("group", ["b2", "b1"])
def test_seq(st, group):
    mem, model = st.mem, st.model
    b = getattr(L, group)
    cases, want = _seq(mem, model, group, 1, None, f"seq {group} k=1")
    assert want[4].all(), want[4]           # k = 1: every case meets seq_ref.margin's condition
    for c, (name, chain, cut, excluded) in enumerate(cases):
        if cut:                             # b1 and b2 begin a source: no chain across them
            assert want[0][c, 0] != chain[-1] and want[2][c, 0].tolist() != list(chain), name
        elif excluded in chain:
            assert excluded not in want[2][c, 0], name
        else:
            assert want[2][c, 0].tolist() == list(chain), (name, want[2][c, 0])
    ends = want[0][:4, 0]                   # the cases at the boundary: answers on both sides of it
    assert (ends >= b).any() and (ends < b).any()
    cases, want = _seq(mem, model, group, B.SEQ_K, B.SEQ_MIN, f"seq {group} k=3")
    for c, (name, chain, cut, excluded) in enumerate(cases):
        if not cut and excluded not in chain:
            assert want[2][c, 0].tolist() == list(chain), (name, want[2][c, 0])
    # the chain at gaps of 2 is no chain with max_step = 1
    cases, want = _seq(mem, model, group, 1, B.SEQ_MIN, f"seq {group} max_step=1", G=1, first=1)
    assert want[2][0, 0].tolist() != list(cases[0][1])


# ---- mutations: each updates the model -------------------------------------------------------------------------------------
def test_append_novel(st):
    mem, model = st.mem, st.model
    plant, n0 = B.planted_rows(L), model.total
    fresh = B.fresh_rows(L)
    dup_of = [L.b2 - 1, L.b2 + 2, L.N - 1]                                # either side of 4 GiB, and the tail
    dups = B.noisy_copy(np.stack([plant[r] for r in dup_of]), 50, noise=0.02)
    batch = np.stack([dups[0], fresh[0], dups[1], fresh[1], dups[2], fresh[2]])
    ks, kr = NV.top1(batch, model.rows, "f16")
    kr = model.gid[kr]
    assert (ks[0::2] > 0.9).all() and kr[0::2].tolist() == dup_of and (ks[1::2] < 0.5).all()    # what the memory's top-1 decides
    keep, row_of = NV.gate(batch, 0.8, "f16", n0, ks, kr)
    assert keep.tolist() == [False, True] * 3 and row_of[1::2].tolist() == [n0, n0 + 1, n0 + 2]
    ids = n0 + np.arange(3)
    tags = B.tag_of(L, ids) + B.LATE_MS                                   # the stored rows come 5 ms late
    got = mem.append_novel(from_bits(batch), 0.8, group=torch.from_numpy(np.repeat(ids // B.GROUP, 2)).cuda(),
                           tag=torch.from_numpy(np.repeat(tags, 2)).cuda())
    assert got.kept == 3 and np_of(got.keep).tolist() == keep.tolist()
    assert np_of(got.row_of).tolist() == row_of.tolist()
    assert len(mem) == n0 + 3
    model.append(batch[1::2], ids // B.GROUP, tags)
    _read_back(mem, model, "append_novel")
    s, r = mem.topk(from_bits(batch[1::2]), 1)
    _pair(s, r, model.topk(batch[1::2], 1), "the rows just stored")
    assert np_of(r)[:, 0].tolist() == ids.tolist()
    # a clip across the old tail, past 4 GiB: found without max_gap_ms, no window once the 6 ms step exceeds it
    clip = B.noisy_copy(np.concatenate([model.rows[model.at(n0 - 2):model.at(n0 - 1) + 1], batch[1:5:2]]), 60)[None]
    for gap, found in ((None, True), (1, False), (B.LATE_MS + 1, True)):
        want = _clip(mem, model, clip, 1, 1, gap, None, f"clip across the old tail, max_gap_ms={gap}")
        assert want[2].all() and (want[0][0, 0] == n0 - 2) == found, (gap, want[0])


def test_erase(st):
    mem, model = st.mem, st.model
    n0 = model.total
    gone = [L.ctrl + 3, L.b1 + 5]              # one row below 2 GiB, one between 2 GiB and 4 GiB
    before = model.gid.copy()
    moved = model.erase(gone)
    out = mem.erase(rows=gone)
    assert out.count == 2 and len(mem) == n0 - 2 == model.total
    assert out.new_row_of.shape[0] == n0
    got = out.new_row_of[torch.from_numpy(before).cuda()].cpu().numpy()
    assert got.tolist() == [moved[int(r)] for r in before], "new_row_of at the sites"
    assert moved[L.b1 + 4] == L.b1 + 3 and moved[L.b2] == L.b2 - 2 and moved[L.ctrl + 2] == L.ctrl + 2
    _read_back(mem, model, "erase")
    _plain(mem, model, 4, "after erase: ")
    _plain(mem, model, 160, "after erase: ")
    _scoped_and_grouped(mem, model, "after erase: ")
    _biased(mem, model, "after erase: ")        # the columns are built anew: the rows behind the erased ones moved a slot
    _fold(mem, model, "max", "after erase: ")
    _seq(mem, model, "b1", 1, None, "after erase: seq b1 k=1")


def test_ring(st):
    """A ring of capacity N after N + 300 rows: the head stands at slot 300, the planted rows 0 and 1 are overwritten, row
    ids run 300 .. N + 299 and row 2^21 still lies at byte offset 2^32."""
    if st.mem is not None:
        st.mem.close()
    st.mem = st.model = None
    torch.cuda.empty_cache()
    st.mem, st.model, REPORT["ring_build_seconds"], REPORT["ring_device_bytes_taken"] = _build(ring=True)
    mem, model = st.mem, st.model
    assert model.base == 300 and model.gid.min() >= 300 and len(mem) == L.N + 300 and mem.searchable == L.N
    _read_back(mem, model, "ring")
    for Q in (4, 160, 800):
        want = _plain(mem, model, Q, "ring: ")
        assert want[0].min() >= 300 and not np.isin(want[0][:2, 0], (0, 1)).any()       # rows 0 and 1 are gone
        assert want[0][0, 0] == B.members(L, 0)[0] and want[0][1, 0] == B.members(L, 1)[0]
    q = B.queries(L, 16, 7)
    for name, (scope, k, _) in B.scope_cases(L).items():
        _both(lambda e: mem.topk_scoped(from_bits(q), k, scope, exact=e), model.scoped(q, scope, k), lambda: mem.last_scope_flags, 16,
              f"ring: scoped {name}")
    _spans(mem, model, "ring: ")
    want = _range(mem, model, "ring: ")
    assert all(w[0].min() >= 300 for w in want)
    # the three newer searches: the columns are read by slot (row id - 300 would be another entry), rows 0 and 1 are gone
    want = _biased(mem, model, "ring: ")
    assert want[0].min() >= 300
    assert _fold(mem, model, "min", "ring: ")[0].min() >= 300
    # the memory goes on for 300 rows behind the last neighbourhood, so the members at its end are no sound chain rows:
    # every sequence's mask leaves them out
    tail = [L.N - 16 + f for f in range(B.FAMILIES)]
    _, want = _seq(mem, model, "b2", 1, None, "ring: seq b2 k=1", without=tail)
    assert want[0][want[0] >= 0].min() >= 300 and not np.isin(want[2], tail).any()


def test_bf16(st):
    """The same recipe in bf16 (the kernels share their addressing through the dtype template): read-back, the plain
    search on the list scan and on the cascade with both 256 x 256 passes, and the scoped search."""
    if st.mem is not None:
        st.mem.close()
    st.mem = st.model = None
    torch.cuda.empty_cache()
    st.mem, st.model, REPORT["bf16_build_seconds"], _ = _build(ring=False, dtype="bf16")
    mem, model = st.mem, st.model
    _read_back(mem, model, "bf16")
    for Q in (4, 800):
        _plain(mem, model, Q, "bf16: ")
    q = B.queries(L, 16, 7, dtype="bf16")
    for name, (scope, k, _) in B.scope_cases(L).items():
        _both(lambda e: mem.topk_scoped(from_bits(q, "bf16"), k, scope, exact=e), model.scoped(q, scope, k),
              lambda: mem.last_scope_flags, 16, f"bf16: scoped {name}")
    _biased(mem, model, "bf16: ")
