"""CPU: the range-search oracle (tests/range_ref.py) against the top-k oracle, its edges, the host-side segmentation
into moments (vidmem.memory.segment_moments) and the declared / bound symbols of the range search."""
import os
import re

import numpy as np
import pytest

from oracle import cref
from tests import range_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN = R.INT64_MIN


def _case(seed, n=600, D=128, Q=8):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n // 6, D))
    rows = (centres[np.arange(n) // 6] + 0.3 * rng.standard_normal((n, D))).astype(np.float16)
    for i in range(0, 60, 7):                        # planted exact duplicates: equal scores on both sides of the cut
        rows[rng.integers(0, n)] = rows[i]
    q = (rows[rng.integers(0, n, Q)].astype(np.float32) + 0.1 * rng.standard_normal((Q, D)).astype(np.float32))
    return q.astype(np.float16).view(np.uint16), rows.view(np.uint16)


# ---- range_ref against the top-k oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("score_mode,min_score", [(0, 0.3), (0, -1.0), (0, 0.95), (1, 0.65), (1, 0.2)])
@pytest.mark.parametrize("seed", [0, 1])
def test_range_ref_is_the_topk_oracle_with_k_equal_n(seed, score_mode, min_score):
    q, rows = _case(seed)
    n = rows.shape[0]
    want_r, want_s = cref.cosine_topk(q, rows, n, dtype="f16", score_mode=score_mode, min_score=min_score)
    got = R.range_hits(q, rows, min_score, dtype="f16", score_mode=score_mode, base=0)
    some = 0
    for qi, (r, s, c) in enumerate(got):
        live = want_r[qi] >= 0
        assert c == int(live.sum()) == r.size
        order = np.argsort(want_r[qi][live], kind="stable")       # re-sorted by row it is the same list
        assert np.array_equal(r, want_r[qi][live][order])
        assert np.array_equal(s.view(np.int64), want_s[qi][live][order].view(np.int64))
        assert (np.diff(r) > 0).all()
        some += c
    assert some > 0 or min_score > 0.9


def test_range_ref_base_scopes_and_padding():
    q, rows = _case(3, n=120)
    tags = np.arange(120, dtype=np.int64) % 10
    tags[5] = MIN
    hits = R.range_hits(q, rows, -1.0, tags=tags, scopes=[(2, 4)] * 4 + [(7, 3), (MIN, MIN), (50, 60), (MIN, R.INT64_MAX)],
                        base=1000)
    assert all(((tags[r - 1000] >= 2) & (tags[r - 1000] <= 4)).all() and c == 36 for r, _, c in hits[:4])
    assert hits[4][2] == 0 and hits[5][0].tolist() == [1005] and hits[6][2] == 0 and hits[7][2] == 120
    rows_p, scores_p, counts = R.padded(hits, 7)
    assert counts.tolist() == [36] * 4 + [0, 1, 0, 120]
    assert rows_p[5].tolist() == [1005] + [-1] * 6 and (scores_p[4] == 0.0).all()
    assert rows_p[7].tolist() == list(range(1000, 1007))


# ---- edges -------------------------------------------------------------------------------------------------------
def test_zero_row_zero_query_and_the_unit_interval_mapping():
    q, rows = _case(4, n=60, Q=3)
    rows = rows.copy()
    q = q.copy()
    rows[17] = 0                                     # a zero row scores 0.0 against everything
    q[2] = 0                                         # a zero query scores 0.0 against every row
    hits = R.range_hits(q, rows, -0.5)
    for r, s, _ in hits[:2]:
        assert 17 in r.tolist() and s[r.tolist().index(17)] == 0.0
    assert hits[2][0].tolist() == list(range(60)) and (hits[2][1] == 0.0).all()
    assert R.range_hits(q, rows, 0.0)[2][2] == 0                    # strict: 0.0 is not above 0.0
    # UNIT_INTERVAL: shown = (1 + cos) / 2, compared after the mapping; the zero row shows 0.5
    m = cref.cosine_matrix(q, rows)
    unit = R.range_hits(q, rows, 0.5, score_mode=1)
    for qi in range(2):
        want = np.nonzero((1.0 + m[qi]) / 2.0 > 0.5)[0]
        assert np.array_equal(unit[qi][0], want) and 17 not in want.tolist()
        assert np.array_equal(unit[qi][1].view(np.int64), ((1.0 + m[qi][want]) / 2.0).view(np.int64))
    assert R.range_hits(q, rows, np.nextafter(0.5, -np.inf), score_mode=1)[2][2] == 60
    # the strict `>` on an exact score
    s = float(m[0, 5])
    assert 5 not in R.range_hits(q, rows, s)[0][0].tolist()
    assert 5 in R.range_hits(q, rows, np.nextafter(s, -np.inf))[0][0].tolist()


# ---- segment_moments ---------------------------------------------------------------------------------------------
def tag(source, ms):
    return (int(source) << 40) | int(ms)


def moments(rows, scores, tags, gap):
    from vidmem.memory import segment_moments
    return segment_moments(np.asarray(rows, np.int64), np.asarray(scores, np.float64), np.asarray(tags, np.int64), gap)


def test_gap_exactly_at_the_limit_joins_and_one_ms_more_splits():
    rows, scores = [10, 11, 12], [0.5, 0.7, 0.6]
    one = moments(rows, scores, [tag(3, 0), tag(3, 100), tag(3, 200)], 100)
    assert len(one) == 1
    assert tuple(one[0]) == (3, 0, 200, 10, 12, 3, 11, 0.7)
    two = moments(rows, scores, [tag(3, 0), tag(3, 100), tag(3, 201)], 100)
    assert [tuple(m) for m in two] == [(3, 0, 100, 10, 11, 2, 11, 0.7), (3, 201, 201, 12, 12, 1, 12, 0.6)]


def test_source_change_with_continuous_milliseconds_splits():
    got = moments([0, 1, 2, 3], [0.9, 0.8, 0.7, 0.6], [tag(1, 0), tag(1, 33), tag(2, 66), tag(2, 99)], 1000)
    assert [(m.source, m.t0_ms, m.t1_ms, m.hits) for m in got] == [(1, 0, 33, 2), (2, 66, 99, 2)]


def test_milliseconds_that_step_backwards_split():
    got = moments([4, 5, 6], [0.3, 0.4, 0.5], [tag(0, 500), tag(0, 499), tag(0, 499)], 1000)
    assert [(m.first_row, m.last_row) for m in got] == [(5, 6), (4, 4)]       # equal milliseconds continue a run
    assert got[0].peak_row == 6


def test_peak_tie_goes_to_the_lower_row():
    got = moments([7, 8, 9, 10], [0.2, 0.9, 0.9, 0.1], [tag(0, i) for i in range(4)], 5)
    assert len(got) == 1 and got[0].peak_row == 8 and got[0].peak_score == 0.9


def test_untimed_rows_are_dropped_and_do_not_break_a_run():
    got = moments([1, 2, 3, 4], [0.5, 0.99, 0.6, 0.4], [tag(2, 0), MIN, tag(2, 40), MIN], 50)
    assert [tuple(m) for m in got] == [(2, 0, 40, 1, 3, 2, 3, 0.6)]
    assert moments([1, 2], [0.5, 0.6], [MIN, MIN], 50) == []


def test_empty_input_and_bad_arguments():
    assert moments([], [], [], 10) == []
    with pytest.raises(ValueError):
        moments([1, 2], [0.5], [tag(0, 0), tag(0, 1)], 10)
    with pytest.raises(ValueError):
        moments([1], [0.5], [tag(0, 0)], -1)


def test_moments_are_ordered_by_peak_then_first_row():
    tags = [tag(0, 0), tag(0, 1000), tag(0, 2000), tag(1, 0), tag(1, 1)]
    got = moments([0, 1, 2, 3, 4], [0.5, 0.8, 0.5, 0.8, 0.1], tags, 10)
    assert [(m.first_row, m.peak_score) for m in got] == [(1, 0.8), (3, 0.8), (0, 0.5), (2, 0.5)]
    assert got[1].last_row == 4 and got[1].hits == 2


# ---- the C ABI and its binding ---------------------------------------------------------------------------------
def test_header_declares_the_range_entries_and_the_binding_carries_them():
    from vidmem import _lib
    text = open(os.path.join(ROOT, "include", "vidmem.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(vm_[a-z0-9_]+)\s*\(", text))
    for name in ("vm_range_workspace_bytes", "vm_range_cosine", "vm_range_cosine_exact"):
        assert name in declared, f"{name} is not declared in include/vidmem.h"
        assert name in _lib.SYMBOLS, f"{name} is missing from _lib.SYMBOLS"
    # additions only: the ABI version did not move
    assert re.search(r"int\s+vm_abi_version\s*\(void\)", text)


def test_host_side_argument_errors_need_no_device():
    from vidmem import similarity
    from vidmem.memory import Moment, RangeHits, RangeResult
    assert Moment._fields == ("source", "t0_ms", "t1_ms", "first_row", "last_row", "hits", "peak_row", "peak_score")
    assert RangeHits._fields == ("counts", "rows", "scores") and RangeResult._fields == ("rows", "scores", "count")
    with pytest.raises(TypeError):                       # score_mode is a required keyword
        similarity.frames_above(None, [0.0], 0.3)
    with pytest.raises(ValueError, match="score_mode"):
        similarity.frames_above(None, [0.0], 0.3, score_mode=7)
