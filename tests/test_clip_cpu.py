"""CPU: the two statements of the clip search's contract (tests/clip_ref.py) against each other and against the
properties the contract promises: peaks at least min_sep apart, min_sep = 1 = the plain ranking of windows, L = 1 and
min_sep = 1 = the scoped row search's oracle, a plateau of identical rows answers with its lowest start."""
import numpy as np
import pytest

from tests import clip_ref as R
from tests import scope_ref

MS = 33


def tags_for(n, sources, gaps=(), untimed=()):
    """n rows in `sources` contiguous videos, MS apart; a 10 s jump after each row of `gaps`; INT64_MIN at `untimed`."""
    per = -(-n // sources)
    i = np.arange(n, dtype=np.int64)
    ms = (i % per) * MS
    for g in gaps:
        ms[(i > g) & (i // per == g // per)] += 10_000
    tags = ((i // per) << 40) | ms
    for u in untimed:
        tags[u] = R.INT64_MIN
    return tags


def small(n, D, dtype, seed):
    return R.scene_video(n, D, dtype, seed)


def equal(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int64), b[1].view(np.int64))


@pytest.mark.parametrize("dtype,D,L,min_sep,k", [("f16", 128, 3, 4, 5), ("f16", 128, 16, 16, 4), ("bf16", 128, 5, 1, 10),
                                                 ("f16", 256, 8, 32, 3), ("bf16", 128, 1, 1, 7)])
def test_two_statements_agree_untagged(dtype, D, L, min_sep, k):
    rows = small(300, D, dtype, 5)
    clips = R.clips_from(rows, dtype, R.pick_starts(300, L, 3, 7), L, 8)
    for kw in (dict(), dict(score_mode=1, min_score=0.7), dict(min_score=0.2, base=1000)):
        a = R.clip_topk(clips, rows, k, min_sep, dtype, **kw)
        b = R.clip_topk_loop(clips, rows, k, min_sep, dtype, **kw)
        assert equal(a, b), kw
    assert (a[0][a[0] >= 0] >= 1000).all()


@pytest.mark.parametrize("L,min_sep,max_gap", [(4, 4, -1), (4, 2, 1000), (16, 16, 1000), (2, 32, -1)])
def test_two_statements_agree_tagged(L, min_sep, max_gap):
    n = 260
    rows = small(n, 128, "f16", 6)
    tags = tags_for(n, 4, gaps=(30, 100), untimed=(10, 11, 150))
    starts = [63, 20, 140, 200]            # 63: straddles the boundary between source 0 and source 1 (rows 64 / 65)
    clips = R.clips_from(rows, "f16", starts, L, 9)
    scopes = [(R.INT64_MIN, R.INT64_MAX), (0, (1 << 40) - 1), ((2 << 40) | 5 * MS, (2 << 40) | 40 * MS), (10, 5)]
    for sc in (None, scopes):
        a = R.clip_topk(clips, rows, 6, min_sep, "f16", tags=tags, scopes=sc, max_gap_ms=max_gap, base=7)
        b = R.clip_topk_loop(clips, rows, 6, min_sep, "f16", tags=tags, scopes=sc, max_gap_ms=max_gap, base=7)
        assert equal(a, b), sc
    per = 65
    got = a[0][0] - 7                      # clip 0 under the whole-memory scope: no window spans two sources
    got = got[got >= 0]
    assert got.size and ((got // per) == ((got + L - 1) // per)).all()
    assert (a[0][3] == -1).all()           # lo > hi


def test_peaks_are_min_sep_apart_and_min_sep_1_is_the_plain_ranking():
    rows = small(400, 128, "f16", 11)
    L = 6
    clips = R.clips_from(rows, "f16", [50, 333], L, 3)
    for min_sep in (2, 6, 17, 32):
        r, _ = R.clip_topk(clips, rows, 30, min_sep, "f16")
        for c in range(2):
            got = np.sort(r[c][r[c] >= 0])
            assert got.size >= 2 and (np.diff(got) >= min_sep).all(), (min_sep, got)
    r1, s1 = R.clip_topk(clips, rows, 12, 1, "f16")
    for c in range(2):
        W = R.window_scores(R.frame_scores(clips[c], rows, "f16"), L)
        idx = np.arange(W.size)
        order = idx[np.lexsort((idx, -W))][:12]
        assert np.array_equal(r1[c], order) and np.array_equal(s1[c].view(np.int64), W[order].view(np.int64))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_single_frame_clip_is_the_scoped_row_search(dtype):
    n = 500
    rows = small(n, 128, dtype, 13)
    tags = tags_for(n, 5)
    clips = R.clips_from(rows, dtype, [5, 120, 499], 1, 4)
    scopes = [(R.INT64_MIN, R.INT64_MAX), (1 << 40, (2 << 40) - 1), (3 << 40, (3 << 40) | 20 * MS)]
    for kw in (dict(), dict(score_mode=1, min_score=0.6)):
        a = R.clip_topk(clips, rows, 10, 1, dtype, tags=tags, scopes=scopes, base=3, **kw)
        want = scope_ref.scoped_topk(clips[:, 0], rows, tags, scopes, 10, dtype=dtype, base=3, **kw)
        assert equal(a, want), kw


def test_plateau_of_identical_rows_answers_with_its_lowest_start():
    rows = small(200, 128, "f16", 17).copy()
    rows[60:100] = rows[60]                # a static scene of 40 identical rows
    L = 8
    clips = R.clips_from(rows, "f16", [70], L, 2)
    for fn in (R.clip_topk, R.clip_topk_loop):
        r, s = fn(clips, rows, 5, 8, "f16")
        assert r[0, 0] == 60               # 33 windows tie bit for bit: the lowest start is the only peak among them
        assert not ((r[0] > 60) & (r[0] <= 92 + 7)).any(), r[0]


def test_short_memory_and_exactly_one_window():
    rows = small(200, 128, "f16", 19)
    clips = R.clips_from(rows, "f16", [0], 8, 2)
    for fn in (R.clip_topk, R.clip_topk_loop):
        r, s = fn(clips, rows[:7], 3, 8, "f16")
        assert (r == -1).all() and (s == 0.0).all()
        r, s = fn(clips, rows[:8], 3, 8, "f16")
        assert r[0].tolist() == [0, -1, -1] and s[0, 0] > 0.9
