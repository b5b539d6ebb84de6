"""GPU: event segmentation (vm_memory_events / vm_memory_regroup_events, csrc/events.hip) against tests/events_ref.py.

Bar: bit equality everywhere - ``out_links`` as int64 views, ``out_event_of``, ``out_first_rows`` with its padding,
``out_n_events``, and after a regroup the key and ordinal columns.  The data sets and their oracle links are made once
(``events_ref.dataset``) and shared; a fresh memory and a wrapped ring over the same rows differ only in which rows are
live.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import events_ref as E
from tests import group_ref as G
from tests.search_checks import RING_CAP, SENT_I, SENT_LINK, events_ws_need, ptr, raw_append_memory, raw_regroup
from tests.support import from_bits, same_bits

pytestmark = pytest.mark.gpu


def raw_events(mem, threshold, gap=-1, max_events=0, links=True, event_of=True, ws_bytes=None, room=3):
    """One call of the C entry on sentinel-filled buffers ``room`` entries longer than the capacity / ``max_events`` ->
    (rc, links, event_of, first_rows, count) as numpy arrays (the whole buffers, sentinels included)."""
    from vidmem import _lib
    need = events_ws_need(mem)
    ws = torch.empty(max(need if ws_bytes is None else ws_bytes, 256), dtype=torch.uint8, device="cuda")
    lk = torch.full((mem.capacity + room,), SENT_LINK, dtype=torch.float64, device="cuda")
    ev = torch.full((mem.capacity + room,), SENT_I, dtype=torch.int64, device="cuda")
    fr = torch.full((max_events + room,), SENT_I, dtype=torch.int64, device="cuda")
    cnt = torch.full((1,), SENT_I, dtype=torch.int64, device="cuda")
    rc = mem.L.vm_memory_events(mem.handle, float(threshold), int(gap), ptr(lk if links else None),
                                ptr(ev if event_of else None), int(max_events), ptr(fr if max_events else None), ptr(cnt),
                                ptr(ws), need if ws_bytes is None else ws_bytes, _lib.current_stream_ptr())
    torch.cuda.synchronize()
    return rc, lk.cpu().numpy(), ev.cpu().numpy(), fr.cpu().numpy(), int(cnt.item())


def check_events(mem, link, flags, base, threshold, gap=-1, max_events=None, label=""):
    """vm_memory_events of ``mem`` against the oracle's links / flags of its live rows."""
    n = flags.size
    seg = E.segment(flags, base)
    width = seg.count + 2 if max_events is None else max_events
    rc, lk, ev, fr, cnt = raw_events(mem, threshold, gap, width)
    assert rc == 0, (label, rc, mem.L.vm_last_error(mem.ctx.handle))
    assert cnt == seg.count, (label, cnt, seg.count)
    assert same_bits(lk[:n], link), f"{label}: links differ (bit-exact bar) at {np.argwhere(lk[:n] != link)[:5].ravel()}"
    assert np.array_equal(ev[:n], seg.event_of), (label, np.argwhere(ev[:n] != seg.event_of)[:5].ravel())
    assert np.array_equal(fr[:width], E.padded_first_rows(seg.first_rows, width)), label
    assert (lk[n:] == SENT_LINK).all() and (ev[n:] == SENT_I).all() and (fr[width:] == SENT_I).all(), label
    return seg


def columns(mem, n=None):
    """(keys, ordinals) over slots [0, n) in slot order."""
    from vidmem.memory import _tensor_from_ptr
    n = mem.capacity if n is None else n
    k = _tensor_from_ptr(mem.L.vm_memory_group_keys(mem.handle), (n,), torch.int64, mem.device).cpu().numpy().copy()
    o = _tensor_from_ptr(mem.L.vm_memory_group_ordinals(mem.handle), (n,), torch.int64, mem.device).cpu().numpy().copy()
    return k, o


def live_columns(mem):
    """(keys, ordinals) of the live rows in row-id order."""
    total, n = len(mem), mem.searchable
    k, o = columns(mem, n)
    if mem.ring and total > mem.capacity:
        head = total % mem.capacity
        k, o = np.roll(k, -head), np.roll(o, -head)
    return k, o


# ---- 1. the three data sets, fresh and wrapped -------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [False, True], ids=["fresh", "ring"])
@pytest.mark.parametrize("name", list(E.SETS))
def test_planted_scenes(name, ring):
    dtype, bits, sizes, link_all = E.dataset(name)
    n = bits.shape[0]
    cap = RING_CAP[name] if ring else None
    mem = raw_append_memory(bits, dtype, capacity=cap, ring=ring, grouped=True)
    lo = n - cap if ring else 0
    base, host = mem.rows_host()
    assert base == lo and np.array_equal(host, bits[lo:])
    planted = E.scene_flags(sizes)
    if ring:        # the oldest event is partly overwritten, and an event straddles the physical wrap (row id = capacity)
        assert not planted[lo] and not planted[cap] and lo < cap < n
    link = link_all[lo:].copy()
    link[0] = 0.0
    flags = E.opens(link, 0.5)
    want = planted[lo:].copy()
    want[0] = True
    assert np.array_equal(flags, want)                                   # threshold 0.5 recovers the planted scenes
    seg = check_events(mem, link, flags, lo, 0.5, label=f"{name} ring={ring}")
    # truncation: the full count and the first max_events rows; max_events = 0 on NULL outputs: the count only
    check_events(mem, link, flags, lo, 0.5, max_events=5, label="truncated")
    rc, lk, ev, fr, cnt = raw_events(mem, 0.5, max_events=0, links=False, event_of=False)
    assert rc == 0 and cnt == seg.count
    assert (lk == SENT_LINK).all() and (ev == SENT_I).all() and (fr == SENT_I).all()
    # the Python entry: trimmed, the full count
    got = mem.events(0.5, with_links=True)
    assert got.count == seg.count and np.array_equal(got.first_rows.cpu().numpy(), seg.first_rows)
    assert np.array_equal(got.event_of.cpu().numpy(), seg.event_of) and same_bits(got.links.cpu().numpy(), link)
    cut = mem.events(0.5, max_events=4)
    assert cut.count == seg.count and cut.first_rows.tolist() == seg.first_rows[:4].tolist() and cut.links is None
    # whole regroup (from_row NULL; in the ring also from_row = lo and below: whole mode)
    want_re = E.regroup(flags, lo)
    for frm in ((None,) if not ring else (None, lo, lo - 5)):
        rc, cnt = raw_regroup(mem, 0.5, from_row=frm)
        assert rc == 0 and cnt == seg.count
        k, o = live_columns(mem)
        assert np.array_equal(k, want_re.keys) and np.array_equal(o, want_re.ordinals), (name, ring, frm)
    # one hit per scene
    q = from_bits(bits[[lo + 3, n // 2 + lo // 2, n - 1]], dtype)
    want_r, want_s, want_k = G.grouped_topk(bits[[lo + 3, n // 2 + lo // 2, n - 1]], bits[lo:], want_re.keys, 10,
                                            dtype=dtype, base=lo)
    s, r, kk = mem.topk_grouped(q, 10)
    assert np.array_equal(r.cpu().numpy(), want_r) and np.array_equal(kk.cpu().numpy(), want_k)
    assert same_bits(s.cpu().numpy(), want_s)
    assert len(set(want_k[0].tolist())) == 10


# ---- 2. small sizes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025])
def test_small_sizes(n):
    dtype, bits, _, link_all = E.dataset("f16_128")
    mem = raw_append_memory(bits[:n], dtype, capacity=max(n, 16), grouped=True)
    if n == 0:          # an empty memory writes the count and nothing else
        rc, lk, ev, fr, cnt = raw_events(mem, 0.5, max_events=4)
        assert rc == 0 and cnt == 0
        assert (lk == SENT_LINK).all() and (ev == SENT_I).all() and (fr == SENT_I).all()
        before = columns(mem)
        assert raw_regroup(mem, 0.5) == (0, 0)
        assert all(np.array_equal(a, b) for a, b in zip(before, columns(mem)))
        got = mem.events(0.5)
        assert got.count == 0 and got.first_rows.numel() == 0 and got.event_of.numel() == 0
        return
    link = link_all[:n]
    flags = E.opens(link, 0.5)
    seg = check_events(mem, link, flags, 0, 0.5, label=f"n={n}")
    check_events(mem, link, flags, 0, 0.5, max_events=max(seg.count - 1, 0), label=f"n={n} cut")
    check_events(mem, link, E.opens(link, 2.0), 0, 2.0, label=f"n={n} all")
    assert raw_regroup(mem, 0.5) == (0, seg.count)
    k, o = columns(mem, n)
    want = E.regroup(flags)
    assert np.array_equal(k, want.keys) and np.array_equal(o, want.ordinals)
    if mem.capacity > n:
        assert not columns(mem)[0][n:].any() and not columns(mem)[1][n:].any()       # nothing beyond the live rows


# ---- 3. the threshold at a link -------------------------------------------------------------------------------------------
def test_threshold_at_a_link_and_special_rows():
    from vidmem import _lib
    dtype, bits_ro, sizes, _ = E.dataset("f16_128")
    bits = bits_ro[:700].copy()
    starts = np.concatenate([[0], np.cumsum(sizes)])
    inside = [int(s) + 2 for s, z in zip(starts, sizes) if z >= 6 and s + z < 700]
    z, d = inside[3], inside[8]
    bits[z] = 0                                       # a zero row: both its links are 0.0
    bits[d + 1] = bits[d]                             # consecutive identical rows: whatever the oracle says
    link = E.links(bits, dtype)
    assert link[z] == 0.0 and link[z + 1] == 0.0 and abs(link[d + 1] - 1.0) < 1e-9
    print(f"link of two identical rows: {link[d + 1]!r}")
    mem = raw_append_memory(bits, dtype)
    r = inside[5] + 1
    tau = float(link[r])
    assert 0.9 < tau < 1.0
    for thr, opens_r in ((tau, True), (float(np.nextafter(tau, -np.inf)), False)):
        flags = E.opens(link, thr)
        assert bool(flags[r]) == opens_r
        check_events(mem, link, flags, 0, thr, label=f"threshold at a link {opens_r}")
    for thr, opens_z in ((0.0, True), (-1e-9, False)):
        flags = E.opens(link, thr)
        assert bool(flags[z]) == opens_z and bool(flags[z + 1]) == opens_z
        check_events(mem, link, flags, 0, thr, label=f"zero row {thr}")
    for thr in (float(link[d + 1]), 1.0, float(np.nextafter(link[d + 1], -np.inf))):
        check_events(mem, link, E.opens(link, thr), 0, thr, label=f"identical rows {thr!r}")
    assert check_events(mem, link, np.ones(700, bool), 0, 2.0, label="2.0").count == 700
    assert check_events(mem, link, E.opens(link, -np.inf), 0, float("-inf"), label="-inf").count == 1
    rc, lk, ev, fr, cnt = raw_events(mem, float("nan"), max_events=4)
    assert rc == _lib.VM_ERR_INVALID and cnt == SENT_I and (lk == SENT_LINK).all() and (fr == SENT_I).all()
    with pytest.raises(ValueError, match="NaN"):
        mem.events(float("nan"))


# ---- 4. tags ----------------------------------------------------------------------------------------------------------------
def test_tag_clauses():
    from vidmem import _lib
    dtype, bits_ro, sizes, link_all = E.dataset("bf16_1024")
    n = 400
    bits, link = bits_ro[:n], link_all[:n]
    MIN = E.INT64_MIN
    starts = np.concatenate([[0], np.cumsum(sizes)])
    long = [int(s) for s, z in zip(starts, sizes) if z >= 12 and s + z < n]       # scenes with room for a cut inside
    ms = np.arange(n, dtype=np.int64) * 40
    src = np.zeros(n, np.int64)
    a, b, c, d, e = long[:5]
    src[a + 3:] += 1                          # a source change inside a scene
    ms[b + 4:] += 5000                        # a gap inside a scene
    ms[c + 5] -= 120                          # time running backwards for one row
    tags = (src << 40) | ms
    tags[d + 2:d + 6] = MIN                   # INT64_MIN mixed in: in, two score-rule rows, out
    tags[e + 1] = MIN                         # a single untimed row: in and out
    mem = raw_append_memory(bits, dtype, tags=tags, grouped=True)
    for gap in (-1, 1000, 40, 39, 0):
        flags = E.opens(link, 0.5, tags, gap)
        assert flags[a + 3] and flags[d + 2] and not flags[d + 3] and flags[d + 6] and flags[e + 1] and flags[e + 2]
        assert bool(flags[b + 4]) == (gap >= 0) and bool(flags[c + 5]) == (gap >= 0)
        assert bool(flags[c + 6]) == (0 <= gap < 160)
        check_events(mem, link, flags, 0, 0.5, gap=gap, label=f"tags gap={gap}")
        assert raw_regroup(mem, 0.5, gap=gap) == (0, int(flags.sum()))
        k, o = columns(mem, n)
        want = E.regroup(flags)
        assert np.array_equal(k, want.keys) and np.array_equal(o, want.ordinals)
    only_tags = E.opens(link, -np.inf, tags, -1)
    assert only_tags.sum() == 1 + 1 + 4
    check_events(mem, link, only_tags, 0, float("-inf"), label="-inf: the tag rules alone")
    # the Python entry and the host helper on its result
    from vidmem.memory import segment_events
    got = mem.events(0.5, max_gap_ms=1000)
    evs = segment_events(got.first_rows.cpu().numpy(), n, 0, mem.tags_host())
    flags = E.opens(link, 0.5, tags, 1000)
    assert len(evs) == got.count == int(flags.sum()) and sum(x.rows for x in evs) == n
    at = [x for x in evs if x.first_row == d + 2][0]
    assert (at.source, at.t0_ms, at.t1_ms, at.last_row) == (None, None, None, d + 5)
    at = [x for x in evs if x.first_row == a + 3][0]
    assert at.source == 1 and at.t0_ms == (a + 3) * 40
    # a gap on an untagged memory
    plain = raw_append_memory(bits[:64], dtype, grouped=True)
    rc, lk, ev, fr, cnt = raw_events(plain, 0.5, gap=0, max_events=4)
    assert rc == _lib.VM_ERR_INVALID and cnt == SENT_I and (ev == SENT_I).all()
    assert raw_regroup(plain, 0.5, gap=1000)[0] == _lib.VM_ERR_INVALID
    with pytest.raises(ValueError, match="tagged"):
        plain.events(0.5, max_gap_ms=5)


# ---- 5. regroup on a linear memory ----------------------------------------------------------------------------------------
def test_regroup_linear_equals_a_fresh_keyed_append_and_the_group_state():
    from vidmem import _lib
    from vidmem.memory import EmbeddingMemory
    dtype, bits_ro, _, link_all = E.dataset("f16_768")
    n = 1500
    bits, link = bits_ro[:n], link_all[:n]
    flags = E.opens(link, 0.5)
    want = E.regroup(flags)
    mem = raw_append_memory(bits, dtype, capacity=n + 8, grouped=True)
    k0, o0 = columns(mem, n)
    assert np.array_equal(k0, -1 - np.arange(n)) and np.array_equal(o0, np.arange(n))      # the plain append's columns
    assert raw_regroup(mem, 0.5) == (0, want.state[0])
    k, o = columns(mem)
    assert np.array_equal(k[:n], want.keys) and np.array_equal(o[:n], want.ordinals)
    assert np.array_equal(mem.group_keys_host(), want.keys)
    assert not k[n:].any() and not o[n:].any()
    fresh = EmbeddingMemory(n + 8, bits.shape[1], dtype, grouped=True)
    fresh.append(from_bits(bits, dtype), group=torch.from_numpy(want.keys))
    fk, fo = columns(fresh)
    assert np.array_equal(fk, k) and np.array_equal(fo, o)
    qb = bits[[5, 700, 1499, 33]]
    want_r, want_s, want_k = G.grouped_topk(qb, bits, want.keys, 10, dtype=dtype)
    for m in (mem, fresh):
        s, r, kk = m.topk_grouped(from_bits(qb, dtype), 10)
        assert np.array_equal(r.cpu().numpy(), want_r) and np.array_equal(kk.cpu().numpy(), want_k)
        assert same_bits(s.cpu().numpy(), want_s)
    scene_of = want.ordinals[want_r[want_r >= 0]]
    assert all(len(set(row)) == len(row) for row in scene_of.reshape(4, -1).tolist())      # one hit per scene
    # the last event is closed: a keyed append with its key still opens a new group ...
    last_key, last_ord = int(want.keys[-1]), int(want.ordinals[-1])
    mem.append(from_bits(bits_ro[n:n + 1], dtype), group=last_key)
    fresh.append(from_bits(bits_ro[n:n + 1], dtype), group=last_key)
    k, o = columns(mem)
    assert (k[n], o[n]) == (last_key, last_ord + 1)
    assert columns(fresh)[1][n] == last_ord                       # where the group was open it was continued
    # ... and a plain append continues the ordinals without a hole
    first = C.c_int64(0)
    mem.ctx.check(mem.L.vm_memory_append(mem.handle, ptr(from_bits(bits_ro[n + 1:n + 3], dtype)), 2, C.byref(first),
                                         _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    k, o = columns(mem)
    assert first.value == n + 1 and o[n + 1:n + 3].tolist() == [last_ord + 2, last_ord + 3]
    assert k[n + 1:n + 3].tolist() == [-1 - (n + 1), -1 - (n + 2)]
    # the Python entry returns the count; a memory that is not grouped is refused
    assert mem.regroup_events(0.5) == int(E.opens(E.links(bits_ro[:n + 3], dtype), 0.5).sum())
    plain = raw_append_memory(bits[:64], dtype)
    before = raw_events(plain, 0.5, max_events=8)
    assert raw_regroup(plain, 0.5) == (_lib.VM_ERR_INVALID, SENT_I)
    with pytest.raises(ValueError, match="grouped"):
        plain.regroup_events(0.5)
    after = raw_events(plain, 0.5, max_events=8)
    assert all(np.array_equal(x, y) for x, y in zip(before[1:4], after[1:4]))


# ---- 6. regroup after an erase ---------------------------------------------------------------------------------------------
def test_regroup_after_erase():
    dtype, bits_ro, sizes, _ = E.dataset("f16_128")
    n = 600
    starts = np.concatenate([[0], np.cumsum(sizes)])
    mid = [i for i, (s, z) in enumerate(zip(starts, sizes)) if 200 < s and s + z < 400 and z >= 3][0]
    gone = list(range(int(starts[mid]), int(starts[mid] + sizes[mid])))            # a whole middle scene
    mem = raw_append_memory(bits_ro[:n], dtype, grouped=True)
    assert mem.erase(rows=gone).count == len(gone)
    keep = np.ones(n, bool)
    keep[gone] = False
    left = np.ascontiguousarray(bits_ro[:n][keep])
    link = E.links(left, dtype)                      # the two neighbours of the erased scene are now adjacent
    flags = E.opens(link, 0.5)
    assert flags[gone[0]]                            # two different scenes met: still a cut
    check_events(mem, link, flags, 0, 0.5, label="after erase")
    want = E.regroup(flags)
    assert raw_regroup(mem, 0.5) == (0, want.state[0])
    k, o = columns(mem, left.shape[0])
    assert np.array_equal(k, want.keys) and np.array_equal(o, want.ordinals)
    # erasing the rows BETWEEN two halves of one scene joins them
    big = [i for i, (s, z) in enumerate(zip(starts, sizes)) if z >= 9 and s + z < 200][0]
    cut = list(range(int(starts[big]) + 2, int(starts[big]) + 5))
    mem2 = raw_append_memory(bits_ro[:n], dtype, grouped=True)
    mem2.erase(rows=cut)
    keep = np.ones(n, bool)
    keep[cut] = False
    left = np.ascontiguousarray(bits_ro[:n][keep])
    link = E.links(left, dtype)
    flags = E.opens(link, 0.5)
    assert not flags[cut[0]]
    check_events(mem2, link, flags, 0, 0.5, label="after an erase inside a scene")


# ---- 7. tail mode ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [False, True], ids=["linear", "ring_not_wrapped"])
def test_tail_regroups_equal_one_whole_regroup(ring):
    from vidmem.memory import EmbeddingMemory
    dtype, bits_ro, _, link_all = E.dataset("f16_128")
    n = 1300
    bits, link = bits_ro[:n], link_all[:n]
    flags = E.opens(link, 0.5)
    want = E.regroup(flags)
    mem = EmbeddingMemory(n + 30, bits.shape[1], dtype, ring=ring, grouped=True)
    rng = np.random.default_rng(9)
    at, calls, opened = 0, 0, 0
    frm_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
    while at < n:
        end = min(n, at + int(rng.integers(1, 41)))
        mem.append(from_bits(bits[at:end], dtype))                    # default group: one key per call - overwritten below
        if calls % 2:
            frm_dev.fill_(at)
            rc, cnt = raw_regroup(mem, 0.5, from_row=frm_dev)
        else:
            rc, cnt = raw_regroup(mem, 0.5, from_row=at)
        assert rc == 0 and cnt == int(flags[at:end].sum()), (at, end, cnt)
        opened += cnt
        at, calls = end, calls + 1
    assert opened == want.state[0] and calls > 40
    k, o = columns(mem)
    assert np.array_equal(k[:n], want.keys) and np.array_equal(o[:n], want.ordinals)
    assert not k[n:].any() and not o[n:].any()
    # from_row >= n touches nothing and reports 0
    for frm in (n, n + 7):
        assert raw_regroup(mem, 2.0, from_row=frm) == (0, 0)
        k2, o2 = columns(mem)
        assert np.array_equal(k2, k) and np.array_equal(o2, o)
    # the state: the last event is closed, so its own key opens a new group
    mem.append(from_bits(bits_ro[n:n + 1], dtype), group=int(want.keys[-1]))
    assert columns(mem)[1][n] == want.ordinals[-1] + 1
    # one whole regroup of another memory leaves the same columns; from_row <= lo is whole mode
    other = raw_append_memory(bits, dtype, capacity=n + 30, ring=ring, grouped=True)
    for frm in (None, 0, -3):
        assert raw_regroup(other, 2.0) == (0, n)               # every row its own event in between
        assert raw_regroup(other, 0.5, from_row=frm) == (0, want.state[0])
        k3, o3 = columns(other, n)
        assert np.array_equal(k3, want.keys) and np.array_equal(o3, want.ordinals)
    # a tail row that does not open an event takes its predecessor's key and ordinal, whatever put them there
    inside = int(np.nonzero(~flags)[0][50])
    assert raw_regroup(other, 2.0) == (0, n)
    assert raw_regroup(other, 0.5, from_row=inside) == (0, int(flags[inside:].sum()))
    k4, o4 = columns(other, n)
    sub = E.regroup_tail(np.arange(n), np.arange(n), flags, inside)
    assert np.array_equal(k4, sub.keys) and np.array_equal(o4, sub.ordinals)
    assert k4[inside] == inside - 1 and o4[inside] == inside - 1


# ---- 8. workspace, repeatability ---------------------------------------------------------------------------------------------
def test_short_workspace_is_refused_and_the_workspace_size_does_not_matter():
    from vidmem import _lib
    dtype, bits_ro, _, link_all = E.dataset("bf16_1024")
    n = 777
    mem = raw_append_memory(bits_ro[:n], dtype, grouped=True)
    need = events_ws_need(mem)
    rc, lk, ev, fr, cnt = raw_events(mem, 0.5, max_events=8, ws_bytes=need - 1)
    assert rc == _lib.VM_ERR_NOMEM and cnt == SENT_I
    assert (lk == SENT_LINK).all() and (ev == SENT_I).all() and (fr == SENT_I).all()
    before = columns(mem)
    assert raw_regroup(mem, 0.5, ws_bytes=need - 1) == (_lib.VM_ERR_NOMEM, SENT_I)
    assert all(np.array_equal(a, b) for a, b in zip(before, columns(mem)))
    outs = [raw_events(mem, 0.5, max_events=100, ws_bytes=b) for b in (need, need + 256, need + 12345)]
    for other in outs[1:]:
        assert other[0] == 0 and other[4] == outs[0][4]
        assert all(np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in zip(outs[0][1:4], other[1:4]))
    flags = E.opens(link_all[:n], 0.5)
    assert outs[0][4] == int(flags.sum())


# ---- 9. graph capture ----------------------------------------------------------------------------------------------------------
def test_graph_capture_append_and_events_replayed():
    from vidmem.memory import EmbeddingMemory
    dtype, bits_ro, _, link_all = E.dataset("f16_768")
    B, H = 128, 64
    mem = EmbeddingMemory(1024, 768, dtype)
    mem.append(from_bits(bits_ro[:256], dtype))
    scratch = mem.prepare_events(H)
    src = from_bits(bits_ro[256:256 + B], dtype).clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            mem.append(src)
            out = mem.enqueue_events(0.5, max_events=H, with_links=True, scratch=scratch)
    torch.cuda.current_stream().wait_stream(s)
    mem.sync()                     # the capture advanced only the host mirror: back to the device count
    assert len(mem) == 256
    for rep in range(3):
        n = 256 + (rep + 1) * B
        src.copy_(from_bits(bits_ro[n - B:n], dtype))
        graph.replay()
        torch.cuda.synchronize()
        assert mem.sync() == n
        link = link_all[:n]
        seg = E.segment(E.opens(link, 0.5))
        assert int(out.count.item()) == seg.count
        assert np.array_equal(out.first_rows.cpu().numpy(), E.padded_first_rows(seg.first_rows, H))
        assert np.array_equal(out.event_of[:n].cpu().numpy(), seg.event_of)
        assert same_bits(out.links[:n].cpu().numpy(), link)
