"""CPU: the host models of tests/compose_ref.py proved against each other, and their case tables shown to tell the right
rules from eight wrong ones (no GPU; tests/test_compose_gpu.py runs the same tables through the kernels).

  identities   the look-ahead group search as the extractor composes it (top-k over the memory, select over the group's
               all-pairs matrix, merge) equals its plain definition, chunk by chunk; row-sharded retrieval as composed
               (per-shard oracle lists with strided ids, merged) equals the oracle over all live rows - bit for bit, on
               every case of the tables
  defects      each planted defect changes the answer of at least one case of every table that is meant to catch it
"""
from __future__ import annotations

import numpy as np
import pytest

from tests import compose_ref as R
from tests import topk_plan as TP
from tests.topk_ref import merge_topk

GROUP_CASES = R.group_cases()
SHARD_CASES = R.all_shard_cases()
_local = {}
_right = {}      # (group case, group) -> the right composition, shared among the defects


def local_lists(c: R.ShardCase, counts=None):
    """One oracle run per (case, step) at the largest k of the case; smaller k are its first columns."""
    key = (c.name, None if counts is None else tuple(counts))
    if key not in _local:
        _local[key] = R.shard_local(c.queries, c.hist, max(c.ks), c.dtype, c.world, counts, c.cap)
    return _local[key]


def shard_runs(c: R.ShardCase):
    """(k, counts) of every search a sharded case makes."""
    for counts in (c.steps or [None]):
        for k in c.ks:
            yield k, counts


# ---------------------------------------------------------------------------------------------------------------------
# the models on inputs small enough to work out by hand
# ---------------------------------------------------------------------------------------------------------------------
def test_select_ref_by_hand():
    inf = np.inf
    m = np.array([[1.0, 3.0, 3.0, -inf, 3.0, 9.0],
                  [0.0, -0.0, 0.0, inf, -1.0, inf]])
    s, r = R.select_ref(m, np.array([5, 6]), 4, row_base=100)
    assert r.tolist() == [[101, 102, 104, 100], [103, 105, 100, 101]]
    assert s[0].tolist() == [3.0, 3.0, 3.0, 1.0] and s[1, :2].tolist() == [inf, inf]
    assert np.signbit(s[1, 2:]).tolist() == [False, True]           # the bits of the selected entries
    s, r = R.select_ref(m, np.array([-3, 1]), 3)
    assert r.tolist() == [[-1, -1, -1], [0, -1, -1]] and s.tolist() == [[0.0] * 3, [0.0] * 3]
    assert R.select_ref(m, None, 2)[1].tolist() == [[5, 1], [3, 5]]
    assert R.select_ref(m, np.array([99, 99]), 2)[1].tolist() == [[5, 1], [3, 5]]   # clamped to S
    # the planted defects, on the same matrix
    assert R.select_ref(m, np.array([5, 6]), 1, inclusive=True)[1].tolist() == [[5], [3]]
    assert R.select_ref(m, np.array([5, 6]), 2, ties_descending=True)[1].tolist() == [[4, 2], [5, 3]]
    assert R.select_ref(m, np.array([2, 2]), 1, ignore_limit=True)[1].tolist() == [[5], [3]]


def test_merge_ref_by_hand():
    s = np.array([[[0.9, 0.5, 0.5]], [[0.9, 0.5, 0.0]], [[0.7, 0.0, 0.0]]])
    r = np.array([[[8, 4, 6]], [[2, 5, -1]], [[-1, -1, -1]]], np.int64)
    ms, mr = R.merge_ref(s, r)
    assert mr.tolist() == [[2, 8, 4]] and ms.tolist() == [[0.9, 0.9, 0.5]]
    assert R.merge_ref(s, r, ties_by_part=True)[1].tolist() == [[8, 2, 4]]
    assert R.merge_ref(s, r, drop_equal=True)[1].tolist() == [[2, 4, -1]]
    # the same (score, row) in two parts: both copies come out, the earlier part's first (seen through the sign of zero)
    zs, zr = R.merge_ref(*R.merge_signed_zero_case())
    assert zr.tolist() == [[5, 5]] and np.signbit(zs).tolist() == [[False, True]]


def test_merge_ref_is_merge_topk():
    """The third sort key (position in the concatenation) is what a stable sort does anyway: on every crafted list,
    the shared-entry ones included, merge_ref equals tests/topk_ref.py::merge_topk."""
    for name, s, r in R.merge_cases():
        k = s.shape[2]
        want_r, want_s = merge_topk([(r[p], s[p]) for p in range(s.shape[0])], k)
        assert R.same(R.merge_ref(s, r), (want_s, want_r)), name


def test_bit_patterns():
    x = np.array([1.0, -2.5, 65504.0, 1e-7, 0.0], np.float32)
    assert R.to_bits(x, "f16").tolist() == x.astype(np.float16).view(np.uint16).tolist()
    # bf16 round to nearest even: 1 + 2^-8 is a tie and goes to the even 1.0, 1 + 3 * 2^-8 to 1 + 2^-6
    y = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -3.3895e38], np.float32)
    assert R.to_bits(y, "bf16").tolist() == [0x3F80, 0x3F80, 0x3F82, 0xFF7F]
    for dtype in ("f16", "bf16", "f32"):
        for D in (R.COS16_D if dtype != "f32" else R.COS32_D):
            q, r = R.cosine_pair(dtype, D)
            for v in (q, r):
                assert not v[R.PLANT_ZERO].any() and np.count_nonzero(v[R.PLANT_ONE]) == 1
                assert np.array_equal(v[R.PLANT_DUP[0]], v[R.PLANT_DUP[1]])
            assert np.array_equal(q[4], r[256]) and q.shape[0] == 70 and r.shape[0] == 600
            if dtype == "f32":
                assert np.isfinite(r).all() and (np.abs(r[R.PLANT_SUB]) < np.finfo(np.float32).tiny).all()
                rnd = r[6:]
                assert not np.array_equal(rnd.astype(np.float16).astype(np.float32)[rnd != 0], rnd[rnd != 0])
                assert ((rnd.view(np.uint32) & 0xFFFF) != 0).all()          # not a bf16 value either
            else:
                exp = {"f16": 0x7C00, "bf16": 0x7F80}[dtype]
                assert ((r & exp) != exp).all() and ((q & exp) != exp).all()   # no inf, no NaN
                assert ((r[R.PLANT_SUB] & exp) == 0).all() and (r[R.PLANT_SUB] & R.SUBNORMAL_MASK[dtype]).all()


# ---------------------------------------------------------------------------------------------------------------------
# identities
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GROUP_CASES, ids=lambda c: c.name)
def test_group_search_identity(c):
    first = 0
    for stored, emb in R.group_walk(c):
        want = R.group_search_ref(stored, emb, c.counts, c.k, c.dtype, first)
        assert R.same(R.group_search_composed(stored, emb, c.counts, c.k, c.dtype, first), want)
        s, r = want
        live = (r >= 0).sum(1)
        starts = R.chunk_starts(c.counts)
        assert (live == np.minimum(c.k, stored.shape[0] + starts)).all()      # what was stored before the chunk
        assert (r.max(1) < stored.shape[0] + starts).all()                    # nothing of the own chunk or later


def test_group_search_identity_with_a_first_row():
    """Row ids offset by first_row: a memory whose first searchable row is not row 0."""
    c = next(c for c in GROUP_CASES if c.mem_kind == "filled" and c.k >= 4 and sum(c.counts) < 30)
    for stored, emb in R.group_walk(c):
        want = R.group_search_ref(stored, emb, c.counts, c.k, c.dtype, first_row=1000)
        assert R.same(R.group_search_composed(stored, emb, c.counts, c.k, c.dtype, first_row=1000), want)
        assert want[1][want[1] >= 0].min() >= 1000


@pytest.mark.parametrize("c", SHARD_CASES, ids=lambda c: c.name)
def test_sharded_identity(c):
    for k, counts in shard_runs(c):
        ps, loc = local_lists(c, counts)
        parts = ps[:, :, :k], R.shard_global(loc[:, :, :k], c.hist.shape[0])
        want = R.sharded_ref(c.queries, c.hist, k, c.dtype, c.world, counts, c.cap)
        assert R.same(R.merge_ref(*parts), want), (k, counts)
        if counts is None:
            for q, ids in c.expect.items():
                assert want[1][q, :min(k, len(ids))].tolist() == ids[:k], (q, k)


def test_oracle_prefix_property():
    """Sharing one oracle run among several k rests on this: the list at k is the head of the list at a larger k."""
    c = next(c for c in SHARD_CASES if c.name == "W3-f16-D256-M1000")
    big = R.shard_parts(c.queries, c.hist, 100, c.dtype, c.world)
    for k in (1, 10, 58):
        assert R.same(R.shard_parts(c.queries, c.hist, k, c.dtype, c.world), (big[0][:, :, :k], big[1][:, :, :k]))


def test_case_tables_hold_what_the_issue_asks():
    names = {c.name for c in SHARD_CASES}
    for W in R.SHARD_W:
        for dtype, D in R.SHARD_TYPES:
            for M in (5, 77, 461, 797, 1000, 20_011):
                assert f"W{W}-{dtype}-D{D}-M{M}" in names
    assert any(len(ids) == 0 for c in SHARD_CASES if c.hist.shape[0] == 5
               for ids in R.shard_live_ids(5, c.world))                                # a shard with no row at all
    ring = next(c for c in SHARD_CASES if c.cap)
    seen = {min(n, ring.cap + 1) for step in ring.steps for n in step}
    assert ring.steps[-1] == [R.RING_FED] * 8 and {1, ring.cap, ring.cap + 1} <= seen   # filling, exactly full, wrapped
    assert any(len(set(step)) > 1 for step in ring.steps)                              # uneven across the shards
    kinds = {(c.mem_kind, c.counts) for c in GROUP_CASES if c.D >= 768}
    assert {m for m, _ in kinds} == set(R.GRP_MEMS) and {n for _, n in kinds} == set(R.GRP_COUNTS)
    for what in ("k", "mem_kind", "counts"):
        for content in R.GRP_CONTENTS:      # every content meets every k, memory kind and counts
            assert ({getattr(c, what) for c in GROUP_CASES if content in c.contents}
                    == {getattr(c, what) for c in GROUP_CASES}), (what, content)
    assert {c.k for c in GROUP_CASES} == set(R.GRP_K)
    for c in GROUP_CASES:
        if c.ring:
            assert c.capacity == c.mem.shape[0] + sum(g.shape[0] for g in c.groups)    # the guard at equality


def test_cascade_case_is_on_the_cascade():
    c = R.cascade_case()
    p = TP.plan(R.CASCADE_Q, R.CASCADE_K, c.D, c.dtype, R.CASCADE_CAP, 256)
    assert p.family == "cascade" and p.launches["topk_scan"] >= 2, p
    assert c.queries.shape[0] == R.CASCADE_Q and c.capacity == R.CASCADE_CAP
    assert min(len(ids) for ids in R.shard_live_ids(c.hist.shape[0], c.world)) >= 3000


# ---------------------------------------------------------------------------------------------------------------------
# planted defects: (table, wrong model) pairs; each must differ from the right model on at least one case
# ---------------------------------------------------------------------------------------------------------------------
def _select_table(**wrong):
    """Cases of the crafted select table the wrong model gets wrong."""
    return [name for name, m, lim, k, base in R.select_cases()
            if not R.same(R.select_ref(m, lim, k, base, **wrong), R.select_ref(m, lim, k, base))]


def _merge_table(**wrong):
    return [name for name, s, r in R.merge_cases() if not R.same(R.merge_ref(s, r, **wrong), R.merge_ref(s, r))]


def _group_table(**wrong):
    out = []
    for c in GROUP_CASES:
        if sum(c.counts) > 256:
            continue            # the 300-frame groups add nothing to tell the rules apart, only oracle time
        for j, (stored, emb) in enumerate(R.group_walk(c)):
            if (c.name, j) not in _right:
                _right[c.name, j] = R.group_search_composed(stored, emb, c.counts, c.k, c.dtype)
            right = _right[c.name, j]
            kw = dict(wrong)
            if kw.pop("rows_from_zero", False):
                kw["group_base"] = 0
            if not R.same(R.group_search_composed(stored, emb, c.counts, c.k, c.dtype, **kw), right):
                out.append(c.name)
                break
    return out


def _shard_table(merge_kw=None, id_kw=None, with_parts=False):
    """Cases whose merged answer (and, ``with_parts``, whose per-shard lists: the GPU test compares both) change."""
    out = []
    for c in SHARD_CASES:
        for k, counts in shard_runs(c):
            ps, loc = local_lists(c, counts)
            ps, loc = ps[:, :, :k], loc[:, :, :k]
            right_r = R.shard_global(loc, c.hist.shape[0])
            wrong_r = R.shard_global(loc, c.hist.shape[0], **(id_kw or {}))
            differs = not R.same(R.merge_ref(ps, wrong_r, **(merge_kw or {})), R.merge_ref(ps, right_r))
            if with_parts:
                differs = differs or not np.array_equal(wrong_r, right_r)
            if differs:
                out.append(c.name)
                break
    return out


DEFECTS = {
    "1-merge-ties-by-part-crafted": lambda: _merge_table(ties_by_part=True),
    "1-merge-ties-by-part-sharded": lambda: _shard_table(merge_kw=dict(ties_by_part=True)),
    "2-merge-drops-an-equal-score-crafted": lambda: _merge_table(drop_equal=True),
    "2-merge-drops-an-equal-score-sharded": lambda: _shard_table(merge_kw=dict(drop_equal=True)),
    "2-merge-drops-an-equal-score-group": lambda: _group_table(merge_kw=dict(drop_equal=True)),
    "3-select-limit-inclusive-crafted": lambda: _select_table(inclusive=True),
    "3-select-limit-inclusive-group": lambda: _group_table(select_kw=dict(inclusive=True)),
    "4-select-ties-column-descending-crafted": lambda: _select_table(ties_descending=True),
    "4-select-ties-column-descending-group": lambda: _group_table(select_kw=dict(ties_descending=True)),
    "5-select-ignores-limit-crafted": lambda: _select_table(ignore_limit=True),
    "5-select-ignores-limit-group": lambda: _group_table(select_kw=dict(ignore_limit=True)),
    "6-group-rows-from-zero": lambda: _group_table(rows_from_zero=True),
    "7-global-id-blocked": lambda: _shard_table(id_kw=dict(blocked_ids=True)),
    "8-padding-through-the-id-mapping": lambda: _shard_table(id_kw=dict(map_padding=True), with_parts=True),
}


@pytest.mark.parametrize("name", sorted(DEFECTS))
def test_planted_defect_is_caught(name):
    caught = DEFECTS[name]()
    print(f"\n[compose] defect {name}: caught by {len(caught)} case(s), e.g. {caught[:3]}")
    assert caught, f"no case of the table tells defect {name} from the right rule"


def test_what_no_table_can_show():
    """Two facts the tables above are built around.  The group search never holds a tie in which the later part (the
    group) has the smaller row id - memory ids come before group ids - so defect 1 is invisible to it; and a padding
    entry sent through the id mapping stays negative (-world + rank < 0), so the merge drops it and only the
    comparison of the per-shard lists themselves can show defect 8."""
    assert _group_table(merge_kw=dict(ties_by_part=True)) == []
    assert _shard_table(id_kw=dict(map_padding=True)) == []
