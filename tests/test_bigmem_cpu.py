"""CPU: the sparse reference of tests/bigmem_ref.py equals the dense one.

The small layout (6,000 rows, D = 128, pretend boundaries at rows 2,048 and 4,096) is built by the recipe of the large one;
for every search family of tests/test_bigmem_gpu.py the oracle over the neighbourhood rows, mapped to row ids, must equal
the same oracle over all 6,000 rows, rows and scores, on the very cases the GPU test runs.  The noise bound must hold for
every row, and an erase must move the model as it moves the dense array.  For the biased, the any/all and the sequence
search the same, with term indices, chains and the sparse ``must`` against ``seq_ref.margin``; one negative per method: an
operand that breaks the proof trips its assertion and no answer comes back.
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import cref
from tests import bias_ref as BR
from tests import bigmem_ref as B
from tests import clip_ref as CL
from tests import diverse_ref as DR
from tests import fold_ref as FR
from tests import seq_ref as SQ
from tests import events_ref as V
from tests import summary_ref as M
from tests import group_ref as G
from tests import group_scope_ref as GS
from tests import mask_ref as MR
from tests import mix_ref as XR
from tests import range_ref as R
from tests import scope_ref as S
from tests import span_ref as SP

L = B.SMALL


@pytest.fixture(scope="module")
def mem():
    bits, sparse = B.dense(L)
    keys = np.arange(L.N) // B.GROUP
    return bits, keys, B.tag_of(L, np.arange(L.N)), sparse


def _eq(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: rows {got[0].tolist()} != {want[0].tolist()}"
    assert np.array_equal(np.asarray(got[1]).view(np.int64), np.asarray(want[1]).view(np.int64)), what + ": scores"
    for a, b in zip(got[2:], want[2:]):
        assert np.array_equal(a, b), what + ": third output"


def test_layout():
    for lay in (B.SMALL, B.BIG):
        pos = B.positions(lay)
        B.hoods(lay)
        for f in range(B.FAMILIES):
            m = B.members(lay, f)
            assert m[0] // B.GROUP == m[6] // B.GROUP and m[0] >= lay.b2       # two of one family in one group above b2
            groups = {r // B.GROUP for r in m.values()}
            assert len(groups) >= B.K + 3
            assert any(r < lay.b1 for r in m.values()) and any(lay.b1 <= r < lay.b2 for r in m.values())
        assert lay.b1 % lay.source_rows == 0 and lay.b2 % lay.source_rows == 0 and lay.ctrl < lay.b1 // 2
        assert lay.N > lay.b2 + 256 and max(pos) == lay.N - 1
    assert B.BIG.N % 16 and B.BIG.N % 256            # a ragged last tile and a ragged last panel
    assert B.BIG.b1 * B.BIG.D * 2 == 1 << 31 and B.BIG.b2 * B.BIG.D * 2 == 1 << 32 and B.BIG.b2 * B.BIG.D == 1 << 31


def test_noise_bound_every_row(mem):
    bits, _, _, sparse = mem
    x = B.from_bits(bits)
    ratio = np.linalg.norm(x[:, :L.D // 2], axis=1) / np.linalg.norm(x, axis=1)
    planted = np.zeros(L.N, bool)
    planted[list(B.positions(L))] = True
    assert (ratio[~planted] <= B.NOISE_BOUND).all()
    q = np.concatenate([B.queries(L, 160, 3), B.clips_of(L).reshape(-1, L.D), B.mix_terms(L).reshape(-1, L.D)])
    assert B.first_half_only(q)
    sc = cref.cosine_matrix(q, np.ascontiguousarray(bits[~planted]), dtype="f16")
    assert np.abs(sc).max() <= B.NOISE_BOUND
    plant = B.planted_rows(L)
    assert all(np.array_equal(bits[r], plant[r]) for r in plant)
    assert np.array_equal(bits[sparse.gid], sparse.rows)


@pytest.mark.parametrize("Q", [4, 20, 60, 160, 800])
def test_topk(mem, Q):
    bits, _, _, sparse = mem
    q = B.queries(L, Q, Q)
    r, s = cref.cosine_topk(q, bits, B.K, dtype="f16")
    _eq(sparse.topk(q, B.K), (r, s), "topk")
    # the planted scores are several hundred cert_eps apart, as the recipe says: the helper's gap condition (a bound from
    # the certificate, asserted inside ``topk``) holds with room
    assert (-np.diff(s, axis=1) > 100 * MR.cert_eps(L.D)).all()


def test_scoped_and_grouped(mem):
    bits, keys, tags, sparse = mem
    q = B.queries(L, 16, 7)
    _eq(sparse.grouped(q, B.K), G.grouped_topk(q, bits, keys, B.K), "grouped")
    for name, (scope, k, gk) in B.scope_cases(L).items():
        _eq(sparse.scoped(q, scope, k), S.scoped_topk(q, bits, tags, scope, k), f"scoped {name}")
        _eq(sparse.grouped_scoped(q, scope, gk), GS.group_scoped_topk(q, bits, keys, tags, scope, gk), f"grouped {name}")
    for f in range(B.FAMILIES):     # levels 0 and 6 share a group: the grouped answer holds level 0 only
        m = B.members(L, f)
        got = sparse.grouped(q, B.K)[0][f].tolist()
        assert m[0] in got and m[6] not in got


def test_masked_and_span(mem):
    bits, _, tags, sparse = mem
    q = B.queries(L, 16, 8)
    ids = B.mask_rows(L)
    _eq(sparse.masked(q, sparse.sel_of_rows(ids, 16), B.K),
        MR.masked_topk(q, bits, np.tile(np.isin(np.arange(L.N), ids), (16, 1)), B.K), "masked rows")
    scope, k, _ = B.scope_cases(L)["sources above b2"]
    _eq(sparse.masked(q, sparse.sel_of_scope(scope, 16), k),
        MR.masked_topk(q, bits, np.tile(S.scope_mask(tags, *scope), (16, 1)), k), "masked scope")
    for name, (fam, spans, k) in B.span_cases(L).items():
        _eq(sparse.span(q[list(fam)], spans, k), SP.span_topk(q[list(fam)], bits, spans, k), f"span {name}")


def test_range(mem):
    bits, _, tags, sparse = mem
    q = B.queries(L, 16, 9)
    scope = B.scope_cases(L)["sources above b2"][0]
    for sc in (None, [scope] * 16):
        got, want = sparse.range(q, B.RANGE_MIN, sc), R.range_hits(q, bits, B.RANGE_MIN, tags, sc)
        for f, (g, w) in enumerate(zip(got, want)):
            _eq((g[0], g[1]), (w[0], w[1]), "range")
            assert g[2] == w[2] == (3 if sc else B.LEVELS + (f < 2))


@pytest.mark.parametrize("min_sep", [1, 4])
@pytest.mark.parametrize("gap", [-1, 1])
def test_clip(mem, min_sep, gap):
    bits, _, tags, sparse = mem
    clips = B.clips_of(L)
    starts, cut = B.clip_cases(L)
    # k = 1: the condition of clip_ref.margin holds for every clip, over the candidates and - the same function - densely
    got = sparse.clip(clips, 1, min_sep, max_gap_ms=gap)
    _eq(got[:2], CL.clip_topk(clips, bits, 1, min_sep, tags=tags, max_gap_ms=gap), "clip k=1")
    assert got[2].all(), got[2]
    worst, held = CL.margin(clips, bits, 1, min_sep, tags=tags, max_gap_ms=gap)
    assert held and worst > 2
    for c, (s, broken) in enumerate(zip(starts, cut)):
        assert (got[0][c, 0] != s) if broken else got[0][c, 0] == s, (c, got[0][c])
    # k = 3 above min_score: few clips have three such peaks
    got = sparse.clip(clips, B.CLIP_K, min_sep, B.CLIP_MIN, max_gap_ms=gap)
    _eq(got[:2], CL.clip_topk(clips, bits, B.CLIP_K, min_sep, tags=tags, max_gap_ms=gap, min_score=B.CLIP_MIN), "clip")
    for c, (s, broken) in enumerate(zip(starts, cut)):
        assert (s not in got[0][c]) if broken else got[0][c, 0] == s, (c, got[0][c])
    for c in np.flatnonzero(got[2]):         # where the sparse condition says "must certify", the dense margin agrees
        worst, held = CL.margin(clips[c:c + 1], bits, B.CLIP_K, min_sep, tags=tags, max_gap_ms=gap)
        assert held and worst > 2, (c, worst, held)


def test_clip_max_gap_decides(mem):
    """The gated append's rows carry tags 5 ms late (tests/test_bigmem_gpu.py): a clip across the old tail is found
    without ``max_gap_ms`` and is no window with ``max_gap_ms = 1``."""
    bits, _, tags, _ = mem
    _, sparse = B.dense(L)
    fresh = B.fresh_rows(L)
    ids = L.N + np.arange(3)
    sparse.append(fresh, ids // B.GROUP, B.tag_of(L, ids) + B.LATE_MS)
    all_bits, all_tags = np.concatenate([bits, fresh]), np.concatenate([tags, B.tag_of(L, ids) + B.LATE_MS])
    clip = B.noisy_copy(all_bits[L.N - 2:L.N + 2], 60)[None]
    for gap, found in ((-1, True), (1, False), (B.LATE_MS + 1, True)):
        got = sparse.clip(clip, 1, 1, max_gap_ms=gap)
        _eq(got[:2], CL.clip_topk(clip, all_bits, 1, 1, tags=all_tags, max_gap_ms=gap), f"clip gap {gap}")
        assert got[2].all() and (got[0][0, 0] == L.N - 2) == found


def test_summaries(mem):
    bits, keys, _, sparse = mem
    dense, got = M.summarize(bits, keys, "f16"), sparse.summaries()
    at = np.searchsorted(dense.keys, got.keys)
    assert np.array_equal(dense.keys[at], got.keys) and got.keys.size >= 50
    for name in M.Summary._fields:
        a, b = getattr(dense, name)[at], getattr(got, name)
        assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b), name


def test_events(mem):
    """Threshold and bound are this layout's (64 noise dims: adjacent noise rows link up to 0.51; the GPU test's 1,024-dim
    rows stay below 0.4 and use 0.5): the reasoning under test is the same."""
    bits, _, tags, sparse = mem
    threshold, bound = 0.54, 0.52
    link, seg = V.events(bits, threshold, "f16", tags, -1)
    inner = np.zeros(L.N, bool)
    for lo, hi in sparse.inner():
        inner[lo:hi] = True
    assert link[~inner].max() < bound                       # the precondition, here from the dense links
    count, event_of, first, closed = sparse.events(threshold, bound)
    assert count == seg.count and closed.size == B.FAMILIES
    assert np.array_equal(event_of, seg.event_of[sparse.gid]) and np.array_equal(first, seg.first_rows[event_of])


def test_mix_and_diverse(mem):
    bits, _, _, sparse = mem
    terms, w = B.mix_terms(L), [B.MIX_W] * 16
    _eq(sparse.mix(terms, w, B.MIX_K), XR.mix_topk(terms, w, bits, None, B.MIX_K), "mix")
    q, lam = B.queries(L, 16, 10), DR.lam_vector(16)
    _eq(sparse.diverse(q, B.DIV_K, B.POOL, lam), DR.diverse_topk(q, bits, None, B.DIV_K, B.POOL, lam), "diverse")


CAP = L.N + L.spare


def _bias_columns(sparse, tags):
    """-> (the model's two columns, the same columns whole: fp32 [2, S] by the builders' restatements over all rows)."""
    rows, values = B.boost_rows(L)
    now = L.N - 1
    cols = [sparse.col_of_rows(rows, values, CAP), sparse.col_of_age(now, B.age_per_ms(L), B.AGE_FILL, CAP)]
    whole = np.stack([BR.bias_from_rows_ref(rows, values, 0, L.N, CAP),
                      BR.bias_from_tags_ref(tags, 0, CAP, now, B.age_per_ms(L), B.AGE_FILL)])
    return cols, whole


def test_biased(mem):
    bits, _, tags, sparse = mem
    cols, whole = _bias_columns(sparse, tags)
    for col, w in zip(cols, whole):         # the model's entries are the builders', and its bounds hold on every other slot
        assert np.array_equal(col.at.view(np.uint32), w[sparse.gid % CAP].view(np.uint32))
        rest = np.delete(w[:L.N], sparse.gid)
        assert (col.lo <= rest).all() and (rest <= col.hi).all()
    assert (whole[1][L.N:] == np.float32(B.AGE_FILL)).all()
    q, betas = B.queries(L, 16, 13), B.bias_weights()
    assert {0.0, -0.5, 2.0 ** -12} <= set(betas) and min(b for b, c in zip(betas, B.BIAS_INDEX) if c == 1) >= 0
    got = sparse.biased(q, cols, B.BIAS_INDEX, betas, B.BIAS_K)
    _eq(got, BR.bias_topk(q, bits, whole, list(B.BIAS_INDEX), betas, None, B.BIAS_K, capacity=CAP), "biased")
    plain = cref.cosine_topk(q, bits, B.BIAS_K, dtype="f16")
    for f, (c, beta) in enumerate(zip(B.BIAS_INDEX, betas)):
        m = B.members(L, f)
        if c not in (0, 1) or beta == 0.0:           # the zero column, a weight of 0: topk bit for bit
            _eq((got[0][f:f + 1], got[1][f:f + 1]), (plain[0][f:f + 1], plain[1][f:f + 1]), f"biased query {f}")
        elif c == 0 and beta == 1.0:                  # a lower level below b2 outranks the higher one above it
            assert got[0][f, 0] == m[4] < L.b2 <= m[0] and m[0] in got[0][f] and plain[0][f, 0] != m[4]
        elif c == 1 and beta == 1.0:                  # age: the tail's member passes the one below b1
            assert got[0][f].tolist().index(m[2]) < got[0][f].tolist().index(m[1])
    assert any(c == 0 and b == 1.0 for c, b in zip(B.BIAS_INDEX, betas)) and any(c == 1 and b == 1.0 for c, b in zip(B.BIAS_INDEX, betas))
    # negative: one positive entry on a noise slot that is no candidate breaks the proof, and no answer comes back
    with pytest.raises(AssertionError, match="outside the candidates"):
        sparse.biased(q, [cols[0]._replace(hi=1.0), cols[1]], B.BIAS_INDEX, betas, B.BIAS_K)


@pytest.mark.parametrize("op", ["max", "min"])
def test_fold(mem, op):
    bits, _, _, sparse = mem
    terms, w = B.fold_cases(L)[op]
    got = sparse.fold(terms, w, B.FOLD_K, op)
    _eq(got, FR.fold_topk(terms, w, bits, None, B.FOLD_K, op), "fold " + op)
    if op == "max":       # more than one term names a query's five best rows; where rows 0 and 1 do not crowd in, all three
        assert all(len(set(t.tolist())) > 1 for t in got[2]) and all(set(t.tolist()) == {0, 1, 2} for t in got[2][2:14]), got[2]
    else:                 # three copies of one family: which one is the worst differs from row to row
        assert set(got[2].ravel().tolist()) == {0, 1, 2}
    assert (got[0] >= L.b2).any(1).all() and (got[0] < L.b1).any(1).all()


def test_fold_min_of_an_absent_family_trips_the_floor(mem):
    _, _, _, sparse = mem
    terms, _ = B.fold_cases(L)["max"]                 # families c, c + 1, c + 2: no row resembles all three
    with pytest.raises(AssertionError, match="fold min"):
        sparse.fold(terms, [[1.0] * 3] * 16, B.FOLD_K, "min")


def _dense_sel(cases):
    return np.stack([np.ones(L.N, bool) if x is None else np.arange(L.N) != x for _, _, _, x in cases])


@pytest.mark.parametrize("group", ["b2", "b1"])
def test_seq(mem, group):
    bits, _, tags, sparse = mem
    cases = B.seq_cases(L)[group]
    steps, sel, dsel = B.seq_steps(L, cases), B.seq_sel(sparse, cases), _dense_sel(cases)
    for k, ms in ((1, None), (B.SEQ_K, B.SEQ_MIN)):
        got = sparse.seq(steps, k, B.SEQ_G, B.SEQ_SEP, sel=sel, min_score=ms)
        _eq(got[:4], SQ.seq_topk(steps, bits, k, B.SEQ_G, B.SEQ_SEP, tags=tags, sel=dsel, min_score=ms), f"seq k={k}")
        for c in np.flatnonzero(got[4]):       # where the sparse condition says "must certify", the dense margin agrees
            worst, held = SQ.margin(steps[c:c + 1], bits, k, B.SEQ_G, B.SEQ_SEP, tags=tags, sel=dsel[c:c + 1])
            assert held and worst > 4, (c, worst, held)
        if k == 1:
            assert got[4].all(), got[4]
        for c, (name, chain, cut, excluded) in enumerate(cases):
            if cut:           # no chain across the source change; without tags it is the answer
                assert got[0][c, 0] != chain[-1] and not any(got[2][c, i].tolist() == list(chain) for i in range(k)), name
                free = SQ.seq_topk(steps[c:c + 1], bits, 1, B.SEQ_G, B.SEQ_SEP)
                assert free[2][0, 0].tolist() == list(chain) and free[1][0, 0] > got[1][c, 0], name
            elif excluded is None:
                assert got[2][c, 0].tolist() == list(chain), (name, got[2][c, 0])
            elif excluded in chain:       # no returned chain holds the excluded row: the answer is another site's
                assert excluded not in got[2][c] and got[2][c, 0].tolist() != list(chain), name
            else:             # a chain may step over a row its mask does not select
                assert got[2][c, 0].tolist() == list(chain) and chain[0] < excluded < chain[-1], name
    # the chain at gaps of 2 needs max_step >= 2: with max_step = 1 another one is the answer
    one = sparse.seq(steps[:1], 1, 1, B.SEQ_SEP, min_score=B.SEQ_MIN)
    _eq(one[:4], SQ.seq_topk(steps[:1], bits, 1, 1, B.SEQ_SEP, tags=tags, min_score=B.SEQ_MIN), "seq max_step=1")
    assert one[2][0, 0].tolist() != list(cases[0][1])


def test_seq_reach_beyond_the_inset_trips(mem):
    _, _, _, sparse = mem
    cases = B.seq_cases(L)["b2"]
    with pytest.raises(AssertionError, match="a planted row within 32 rows"):
        sparse.seq(B.seq_steps(L, cases), 1, 16, B.SEQ_SEP)


def test_erase_moves_the_model(mem):
    bits, keys, tags, _ = mem
    _, sparse = B.dense(L)
    gone = [L.ctrl + 3, L.b1 + 5]
    moved = sparse.erase(gone)
    keep = ~np.isin(np.arange(L.N), gone)
    assert moved[L.ctrl + 3] == -1 and moved[L.b1 + 4] == L.b1 + 3 and moved[L.b2] == L.b2 - 2 and moved[L.N - 1] == L.N - 3
    assert np.array_equal(bits[keep][sparse.gid], sparse.rows) and sparse.total == L.N - 2
    q = B.queries(L, 16, 11)
    _eq(sparse.topk(q, B.K), cref.cosine_topk(q, np.ascontiguousarray(bits[keep]), B.K, dtype="f16"), "topk after erase")
    scope, k, _ = B.scope_cases(L)["window across b2"]
    _eq(sparse.scoped(q, scope, k), S.scoped_topk(q, bits[keep], tags[keep], scope, k), "scoped after erase")


@pytest.mark.parametrize("boundary", ["b1", "b2"])
def test_a_wrapped_offset_would_show(mem, boundary):
    """What a kernel whose offset wraps at the boundary would read: row r >= b comes from row r - b.  For the rows just
    above b those are rows 0 .. 47 of the first neighbourhood, so the model can say what such a kernel would answer: the
    planted members above the boundary are gone from the answers."""
    import copy
    _, _, _, sparse = mem
    b = getattr(L, boundary)
    wrong = copy.copy(sparse)
    wrong.rows = sparse.rows.copy()
    for r in range(b, b + B.HOOD):
        wrong.rows[sparse.at(r)] = sparse.rows[sparse.at(r - b)]
    q = B.queries(L, 16, 12)
    good, good_s = sparse.topk(q, B.LEVELS)      # every member of the family
    bad, bad_s = cref.cosine_topk(q, np.ascontiguousarray(wrong.rows), B.LEVELS, dtype="f16")
    bad = wrong._ids(bad)
    assert ((good != bad) | (good_s != bad_s)).any(axis=1).all()      # every family's answer changes, in rows or scores
    above = {f: B.members(L, f)[0 if boundary == "b2" else 5] for f in range(B.FAMILIES)}
    for f in range(2, B.FAMILIES):      # (families 0 and 1 would find their copies of rows 0 and 1 there instead)
        assert above[f] in good[f] and above[f] not in bad[f]
    # the three newer searches: every family has a member in [b, b + 48), and each expectation over all of a family's
    # members changes when those rows are read from r - b
    differ = lambda a, b_: ((a[0] != b_[0]) | (a[1].view(np.int64) != b_[1].view(np.int64))).any(axis=1)
    tags = B.tag_of(L, np.arange(L.N))
    cols, _ = _bias_columns(sparse, tags)
    betas = B.bias_weights()
    good = sparse.biased(q, cols, B.BIAS_INDEX, betas, B.LEVELS)
    e = cref.cosine_matrix(q, np.ascontiguousarray(wrong.rows), dtype="f16")
    b_at = np.stack([cols[c].at if c in (0, 1) else np.zeros_like(cols[0].at) for c in B.BIAS_INDEX])
    bad = BR.bias_topk_from_cosines(e, betas, b_at, None, B.LEVELS)
    assert differ(good, (wrong._ids(bad[0]), bad[1])).all()
    terms, w = B.fold_cases(L)["min"]       # three copies of one family for both ops: all nine members are returned
    for op in ("max", "min"):
        good = sparse.fold(terms, w, B.LEVELS, op)
        bad = FR.fold_topk(terms, w, wrong.rows, None, B.LEVELS, op)
        assert differ(good, (wrong._ids(bad[0]), bad[1])).all(), op
    cases = B.seq_cases(L)[boundary]
    steps, sel = B.seq_steps(L, cases), B.seq_sel(sparse, cases)
    good = sparse.seq(steps, 1, B.SEQ_G, B.SEQ_SEP, sel=sel, min_score=B.SEQ_MIN)
    bad = wrong.seq(steps, 1, B.SEQ_G, B.SEQ_SEP, sel=sel, min_score=B.SEQ_MIN)
    for c, (name, chain, cut, _) in enumerate(cases):       # every case whose answer has a row at or above the boundary
        if b <= good[0][c, 0] < b + B.HOOD:
            assert good[2][c, 0].tolist() != bad[2][c, 0].tolist(), name
    assert sum(b <= r < b + B.HOOD for r in good[0][:, 0]) >= 2


def test_bf16_recipe():
    """The bf16 case of the GPU test: the same recipe rounded to bf16, the plain and the scoped search."""
    import torch
    gen = torch.Generator(device="cpu").manual_seed(3)
    cand, parts = {}, []
    for start, x, _, _ in B.blocks(L, gen, "cpu", dtype="bf16"):
        B.cut_hoods(L, start, x, cand)
        parts.append(x.view(torch.int16).numpy().view(np.uint16).copy())
    bits, sparse = np.concatenate(parts), B.Sparse(L, cand, dtype="bf16")
    for Q in (4, 800):
        q = B.queries(L, Q, Q, dtype="bf16")
        _eq(sparse.topk(q, B.K), cref.cosine_topk(q, bits, B.K, dtype="bf16"), "bf16 topk")
    q, tags = B.queries(L, 16, 7, dtype="bf16"), B.tag_of(L, np.arange(L.N))
    for name, (scope, k, _) in B.scope_cases(L).items():
        _eq(sparse.scoped(q, scope, k), S.scoped_topk(q, bits, tags, scope, k, dtype="bf16"), f"bf16 scoped {name}")
