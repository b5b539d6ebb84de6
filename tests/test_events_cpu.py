"""CPU: the event-segmentation oracle (tests/events_ref.py) on planted scenes, the host helper
``vidmem.memory.segment_events``, the ``memory.group_by: event`` configuration and the argument rules of the Python
entries, which are checked before anything reaches the library."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import events_ref as E
from tests.host_memory import host_memory as _host_memory

MIN = E.INT64_MIN


def tag(source, ms):
    return (source << 40) | ms


# ---- the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.SETS))
def test_reference_recovers_planted_scenes(name):
    dtype, bits, sizes, link = E.dataset(name)
    flags = E.scene_flags(sizes)
    assert bits.shape[0] == {"f16_768": 4864, "bf16_1024": 1808, "f16_128": 3542}[name]
    assert link[0] == 0.0
    assert link[~flags].min() > 0.99 and link[flags][1:].max() < 0.35       # scenes are tight and far from each other
    got = E.opens(link, 0.5)
    assert np.array_equal(got, flags)
    seg = E.segment(got, base=7)
    assert seg.count == len(sizes) and seg.first_rows[0] == 7
    assert np.array_equal(np.bincount(seg.event_of), np.array(sizes))
    re = E.regroup(got)
    assert np.array_equal(re.keys, np.repeat(np.concatenate([[0], np.cumsum(sizes)[:-1]]), sizes))
    assert re.state == (len(sizes), int(re.keys[-1]), 0)


def test_links_are_symmetric_and_independent_of_the_block():
    dtype, bits, _, link = E.dataset("f16_128")
    part = bits[:70]
    from oracle import cref
    m = cref.cosine_matrix(part, part, dtype=dtype)
    assert np.array_equal(np.diagonal(m, 1).view(np.int64), np.diagonal(m, -1).view(np.int64))      # both ways, bit for bit
    assert np.array_equal(np.diagonal(m, 1).view(np.int64), link[1:70].view(np.int64))


def test_rule_strictness_thresholds_and_tags():
    link = np.array([0.0, 0.9, 0.5, 0.9, 0.9, 0.9, 0.9, 0.9])
    assert E.opens(link, 0.5).tolist() == [True, False, True] + [False] * 5          # equal to the threshold opens
    assert E.opens(link, np.nextafter(0.5, -1)).tolist() == [True] + [False] * 7
    assert E.opens(link, 2.0).all() and E.opens(link, -np.inf).sum() == 1
    tags = np.array([tag(0, 0), tag(0, 10), tag(0, 20), tag(1, 30), MIN, MIN, tag(1, 5), tag(1, 5000)], np.int64)
    #                                        score      source    one MIN  both MIN  one MIN     gap only
    assert E.opens(link, 0.5, tags, -1).tolist() == [True, False, True, True, True, False, True, False]
    assert E.opens(link, 0.5, tags, 4994).tolist() == [True, False, True, True, True, False, True, True]
    assert E.opens(link, 0.5, tags, 4995).tolist() == [True, False, True, True, True, False, True, False]
    back = np.array([tag(2, 50), tag(2, 40), tag(2, 40)], np.int64)                     # time running backwards
    assert E.opens(link[:3] + 0.95, 0.5, back, 0).tolist() == [True, True, False]
    assert E.opens(link[:3] + 0.95, 0.5, back, -1).tolist() == [True, False, False]
    # -inf leaves only the tag rules
    assert E.opens(link, -np.inf, tags, -1).tolist() == [True, False, False, True, True, False, True, False]


def test_tail_regroup_equals_whole_regroup():
    rng = np.random.default_rng(3)
    flags = rng.random(500) < 0.2
    flags[0] = True
    whole = E.regroup(flags)
    keys, ords, at = whole.keys[:1].copy(), whole.ordinals[:1].copy(), 1
    while at < 500:
        step = int(rng.integers(1, 41))
        end = min(500, at + step)
        grown_k = np.concatenate([keys, np.full(end - at, -99)])
        grown_o = np.concatenate([ords, np.full(end - at, -99)])
        out = E.regroup_tail(grown_k, grown_o, flags[:end], at)
        keys, ords, at = out.keys, out.ordinals, end
    assert np.array_equal(keys, whole.keys) and np.array_equal(ords, whole.ordinals) and out.state == whole.state


# ---- segment_events ----------------------------------------------------------------------------------------------------
def test_segment_events_on_hand_made_tags():
    from vidmem.memory import Event, segment_events
    tags = np.array([tag(0, 0), tag(0, 33), tag(0, 66),          # one event of source 0
                     tag(1, 0), tag(1, 33),                      # a source change
                     tag(1, 9000), tag(1, 9033),                 # a gap
                     tag(1, 100),                                # time running backwards
                     MIN, MIN,                                   # INT64_MIN mixed in: an event of its own
                     tag(1, 200)], np.int64)
    link = np.array([0.0] + [0.9] * 10)
    flags = E.opens(link, 0.5, tags, 1000)
    assert np.nonzero(flags)[0].tolist() == [0, 3, 5, 7, 8, 10]
    first = 100 + np.nonzero(flags)[0]
    got = segment_events(first, 11, base=100, tags=tags)
    assert got == [Event(0, 0, 66, 100, 102, 3), Event(1, 0, 33, 103, 104, 2), Event(1, 9000, 9033, 105, 106, 2),
                   Event(1, 100, 100, 107, 107, 1), Event(None, None, None, 108, 109, 2), Event(1, 200, 200, 110, 110, 1)]
    plain = segment_events(first, 11, base=100)
    assert [(e.first_row, e.last_row, e.rows) for e in plain] == [(e.first_row, e.last_row, e.rows) for e in got]
    assert all(e.source is None and e.t0_ms is None and e.t1_ms is None for e in plain)
    assert segment_events([], 0) == []
    assert segment_events([0], 1) == [Event(None, None, None, 0, 0, 1)]
    for bad in (([1], 3, 0), ([0, 0], 3, 0), ([0, 3], 3, 0), ([], 2, 0), ([5, 4], 9, 5)):
        with pytest.raises(ValueError):
            segment_events(bad[0], bad[1], base=bad[2])
    with pytest.raises(ValueError, match="tags"):
        segment_events([0], 2, tags=[1, 2, 3])


# ---- configuration -----------------------------------------------------------------------------------------------------
def test_config_defaults_and_validation():
    from vidmem import config as cfgmod
    from vidmem import extractor as X
    assert cfgmod.MEMORY_DEFAULTS["event_threshold"] is None and cfgmod.MEMORY_DEFAULTS["event_max_gap_ms"] is None
    cfg = cfgmod.from_dict({"memory": {"group_by": "event", "event_threshold": 0.5}})
    assert cfg.memory.group_by == "event" and cfg.memory.event_max_gap_ms is None and cfg.memory.tag_by is None
    assert X.event_rule(cfg.memory) == (0.5, None)
    assert X.event_rule(cfgmod.from_dict({}).memory) is None
    assert X.event_rule(cfgmod.from_dict({"memory": {"group_by": "chunk"}}).memory) is None
    timed = cfgmod.from_dict({"memory": {"group_by": "event", "event_threshold": 0.5, "event_max_gap_ms": 2000,
                                         "tag_by": "time"}})
    assert X.event_rule(timed.memory) == (0.5, 2000)
    for bad in ({"group_by": "event"}, {"group_by": "event", "event_threshold": "0.5"},
                {"group_by": "event", "event_threshold": float("nan")}, {"group_by": "event", "event_threshold": True}):
        with pytest.raises(ValueError, match="event_threshold"):
            X.event_rule(cfgmod.from_dict({"memory": bad}).memory)
    with pytest.raises(ValueError, match="event_max_gap_ms"):
        X.event_rule(cfgmod.from_dict({"memory": {"group_by": "event", "event_threshold": 0.5,
                                                  "event_max_gap_ms": 10}}).memory)          # a gap without tags
    with pytest.raises(ValueError, match="event_max_gap_ms"):
        X.event_rule(cfgmod.from_dict({"memory": {"group_by": "event", "event_threshold": 0.5, "tag_by": "time",
                                                  "event_max_gap_ms": -5}}).memory)


def test_build_memory_accepts_event_and_still_rejects_scene(monkeypatch):
    from vidmem import config as cfgmod
    from vidmem import extractor as X
    made = []

    class FakeMemory:
        def __init__(self, *a, **kw):
            made.append(kw)

    monkeypatch.setattr(X, "EmbeddingMemory", FakeMemory)
    enc = SimpleNamespace(dtype_name="f16", out_dim=768, device=SimpleNamespace(index=0))
    X.build_memory(cfgmod.from_dict({"memory": {"group_by": "event", "event_threshold": 0.5}}).memory, enc)
    X.build_memory(cfgmod.from_dict({"memory": {"group_by": "chunk"}}).memory, enc)
    X.build_memory(cfgmod.from_dict({}).memory, enc)
    assert [m["grouped"] for m in made] == [True, True, False] and not any(m["tagged"] for m in made)
    with pytest.raises(ValueError, match="event_threshold"):
        X.build_memory(cfgmod.from_dict({"memory": {"group_by": "event"}}).memory, enc)
    for other in ("scene", "events", ""):
        with pytest.raises(ValueError, match="group_by"):
            X.build_memory(cfgmod.from_dict({"memory": {"group_by": other, "event_threshold": 0.5}}).memory, enc)
    assert len(made) == 3


# ---- argument rules of the Python entries -----------------------------------------------------------------------------
def test_argument_errors_are_raised_without_a_library_call():
    plain, grouped, both = _host_memory(), _host_memory(grouped=True), _host_memory(grouped=True, tagged=True)
    for mem in (plain, grouped, both):
        for call in (mem.enqueue_events, mem.events):
            with pytest.raises(ValueError, match="NaN"):
                call(float("nan"))
    with pytest.raises(ValueError, match="NaN"):
        both.regroup_events(float("nan"))
    for call in (plain.enqueue_events, plain.events, grouped.enqueue_events, grouped.enqueue_regroup_events,
                 grouped.regroup_events):
        with pytest.raises(ValueError, match="tagged"):
            call(0.5, max_gap_ms=1000)
    for call in (plain.enqueue_regroup_events, plain.regroup_events):
        with pytest.raises(ValueError, match="grouped"):
            call(0.5)
    with pytest.raises(ValueError, match="max_events"):
        both.enqueue_events(0.5, max_events=-1)
    # what passes the checks goes on to the library
    with pytest.raises(AssertionError, match="library call"):
        both.enqueue_regroup_events(0.5, max_gap_ms=1000)
    with pytest.raises(AssertionError, match="library call"):
        plain.enqueue_events(0.5, max_gap_ms=-1)


def test_symbols_are_declared_and_bound():
    import os
    import re
    from vidmem import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "vidmem.h")).read(), flags=re.S)
    for name in ("vm_memory_events_workspace_bytes", "vm_memory_events", "vm_memory_regroup_events",
                 "vm_memory_group_ordinals"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in _lib.SYMBOLS
