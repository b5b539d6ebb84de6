"""GPU: the clip search (vm_topk_cosine_clip, csrc/topk_clip.hip) against tests/clip_ref.py.

Bar: start rows, fp64 score bits and padding identical to statement (A), for the fast and the ``exact=True`` entry on every
case.  Data: the scene-structured "video" of tests/clip_ref.py (scenes of 24 - 40 rows, row = normalise(centre + 0.5 x unit
noise)); clips are L consecutive stored rows plus 0.1 x unit noise.

Certified condition: on that data the fast path must answer every clip (flag 0) wherever a case says certified.  The
reference alone stays inside that condition.  ``clip_ref.margin`` on the shapes used here, with the bit-exact oracle: the
exact k-th peak cleared the (M+1)-th window that could be a possible peak by (in units of eps_w(D) = cert_eps(D) + 2^-23;
the certificate needs more than 2), and the best M such windows always held k exact peaks:
  4,000 rows, C = 5   (D, L, min_sep, k, dtype): (768, 16, 16, 10, f16) 46.1; (768, 16, 1, 10, f16) 14.8;
                      (1024, 8, 8, 10, f16) 53.7; (128, 3, 32, 10, f16) 1,674; (768, 5, 5, 20, f16) 23.3;
                      (1024, 8, 8, 10, bf16) 53.4
  20,000 rows x 128, L = 16, min_sep = 16, C = 2: k = 1: 49,448; k = 3: 1,770
  70,000 rows x 128, L = 8, min_sep = 8, C = 2: k = 1: 47,466; k = 3: 3,336
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import clip_ref as R
from tests import domain_ref
from tests.search_checks import make_memory
from tests.support import ALL, MS, contiguous_tags, from_bits, scope_of

pytestmark = pytest.mark.gpu


# (D, L, min_sep, k, dtype) at 4,000 rows, C = 5 (odd: the two-clips-per-block scan sees a ragged last pair)
PARITY = [(768, 16, 16, 10, "f16"), (768, 16, 1, 10, "f16"), (1024, 8, 8, 10, "f16"), (128, 3, 32, 10, "f16"),
          (768, 5, 5, 20, "f16"), (1024, 8, 8, 10, "bf16")]
# (rows, D, L, min_sep): above the 16,384-slot cut sample; several compaction slices and appends of 65,536
SIZES = [(20000, 128, 16, 16), (70000, 128, 8, 8)]


def parity_case(D, L, min_sep, k, dtype):
    rows = R.scene_video(4000, D, dtype, 100 + D)
    return rows, R.clips_from(rows, dtype, R.pick_starts(4000, L, 5, L + min_sep), L, k)


def size_case(n, D, L):
    rows = R.scene_video(n, D, "f16", 200 + D)
    return rows, R.clips_from(rows, "f16", R.pick_starts(n, L, 2, n), L, 3)


def same(got_r, got_s, want_r, want_s, what=""):
    assert np.array_equal(got_r, want_r), (what, np.argwhere(got_r != want_r)[:5], got_r[:2], want_r[:2])
    assert np.array_equal(got_s.view(np.int64), want_s.view(np.int64)), f"scores differ (bit-exact bar) {what}"


def check(mem, clips, k, min_sep, dtype, scopes=None, max_gap_ms=None, min_score=None, score_mode=0, certified=False,
          want=None, label=""):
    """Fast and exact entry against statement (A).  certified=True: the fast path answered every clip (flag 0).
    -> (rows, scores, flags) of the fast entry."""
    base, host_rows = mem.rows_host()
    tags = mem.tags_host() if mem.tagged else None
    if want is None:
        want = R.clip_topk(clips, host_rows, k, min_sep, dtype, tags=tags, scopes=scopes,
                           max_gap_ms=-1 if max_gap_ms is None else max_gap_ms, score_mode=score_mode,
                           min_score=min_score, base=base)
    out = None
    for exact in (False, True):
        s, r = mem.topk_clip(from_bits(clips, dtype), k, min_sep=min_sep, scope=scopes, max_gap_ms=max_gap_ms,
                             min_score=min_score, score_mode=score_mode, exact=exact)
        got_r, got_s = r.cpu().numpy(), s.cpu().numpy()
        if not exact:
            flags = mem.last_clip_flags[:clips.shape[0]].cpu().numpy()
            print(f"{label} k={k} C={clips.shape[0]} flagged={int((flags != 0).sum())}")
            out = (got_r, got_s, flags)
        same(got_r, got_s, want[0], want[1], f"{label} exact={exact}")
        if certified and not exact:
            assert (flags == 0).all(), f"fast path flagged {int((flags != 0).sum())} of {clips.shape[0]} clips: {flags}"
    return out


# ---- 1. identity: a one-frame clip with min_sep = 1 is the row search -----------------------------------------------
@pytest.mark.parametrize("D", [128, 768])
def test_one_frame_clip_equals_topk(D):
    rows = R.scene_video(4000, D, "f16", 100 + D)
    mem = make_memory(rows, "f16")
    clips = R.clips_from(rows, "f16", R.pick_starts(4000, 1, 5, 1), 1, 2)
    q = from_bits(clips, "f16")
    s0, r0 = mem.topk(q[:, 0].contiguous(), 10)
    for exact in (False, True):
        s1, r1 = mem.topk_clip(q, 10, min_sep=1, exact=exact)
        same(r1.cpu().numpy(), s1.cpu().numpy(), r0.cpu().numpy(), s0.cpu().numpy(), f"exact={exact}")
    check(mem, clips, 10, 1, "f16")


# ---- 2. parity, certified ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,L,min_sep,k,dtype", PARITY)
def test_parity_certified(D, L, min_sep, k, dtype):
    rows, clips = parity_case(D, L, min_sep, k, dtype)
    mem = make_memory(rows, dtype)
    got_r, _, _ = check(mem, clips, k, min_sep, dtype, certified=True, label=f"parity {dtype} D={D} L={L} sep={min_sep}")
    starts = R.pick_starts(4000, L, 5, L + min_sep)
    assert abs(int(got_r[0, 0]) - starts[0]) < max(min_sep, 2)      # the clip finds the moment it was cut from
    for c in range(5):
        live = np.sort(got_r[c][got_r[c] >= 0])
        assert (np.diff(live) >= min_sep).all()


# ---- 3. selection at size, certified ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,L,min_sep", SIZES)
def test_selection_at_size_certified(n, D, L, min_sep):
    rows, clips = size_case(n, D, L)
    mem = make_memory(rows, "f16")
    want = R.clip_topk(clips, rows, 3, min_sep, "f16")
    check(mem, clips, 3, min_sep, "f16", certified=True, want=want, label=f"size {n}")
    # without a filter the k = 1 answer is the first column of the k = 3 answer (one ranking of the peaks)
    check(mem, clips, 1, min_sep, "f16", certified=True, want=(want[0][:, :1], want[1][:, :1]), label=f"size {n}")


# ---- 4. tags ----------------------------------------------------------------------------------------------------------
def test_tags_no_window_spans_two_videos():
    n, L = 2000, 16
    rows = R.scene_video(n, 128, "f16", 31)
    tags = contiguous_tags(n, 8)                        # 8 sources of 250 rows
    mem = make_memory(rows, "f16", tags=tags, grouped=True)
    clips = R.clips_from(rows, "f16", [242, 700, 1493, 30, 1984], L, 5)   # 242, 1493: planted across a boundary
    for min_sep in (1, 16):
        got_r, _, _ = check(mem, clips, 10, min_sep, "f16", label="sources")
        live = got_r[got_r >= 0]
        assert ((live // 250) == ((live + L - 1) // 250)).all()
        assert 242 not in got_r[0] and 1493 not in got_r[2]
    # the untagged twin of the same rows does return the straddling windows
    plain = make_memory(rows, "f16")
    got_r, _, _ = check(plain, clips, 10, 16, "f16", label="untagged twin")
    assert got_r[0, 0] == 242 and got_r[2, 0] == 1493


def test_tags_max_gap_and_untimed_rows():
    n, L = 1500, 8
    rows = R.scene_video(n, 128, "f16", 33)
    tags = contiguous_tags(n, 3)
    per = n // 3
    i = np.arange(n)
    tags[(i % per) > 100] += 5000                       # a 5 s jump after row 100 of every source
    tags[(i % per) > 300] -= 2000                       # the clock runs backwards after row 300
    tags[40:44] = R.INT64_MIN                           # untimed rows: a window may lie inside them, not across their ends
    tags[900] = R.INT64_MIN
    mem = make_memory(rows, "f16", tags=tags)
    clips = R.clips_from(rows, "f16", [97, 297, 38, 40, 896, 1200], L, 7)
    for gap in (None, 1000, 0):
        check(mem, clips, 8, 8, "f16", max_gap_ms=gap, label=f"max_gap_ms={gap}")
        check(mem, clips[:, :4].copy(), 8, 3, "f16", max_gap_ms=gap, label=f"L=4 max_gap_ms={gap}")
    got_r, _, _ = check(mem, clips, 8, 8, "f16", max_gap_ms=1000)
    assert 97 not in got_r[0] and 297 not in got_r[1]
    got_r, _, _ = check(mem, clips, 8, 8, "f16")
    assert got_r[0, 0] == 97 and got_r[1, 0] == 297 and 38 not in got_r[2]
    got_r, _, _ = check(mem, clips[:, :4].copy(), 8, 3, "f16")
    assert got_r[3, 0] == 40                            # rows 40 .. 43 are all untimed: one valid window


def test_tags_mixed_scopes_in_one_call():
    n, L, k = 2000, 8, 6
    rows = R.scene_video(n, 128, "f16", 35)
    tags = contiguous_tags(n, 8)
    mem = make_memory(rows, "f16", tags=tags)
    # no row at all, lo > hi, fewer than L rows, a sub-window of a video, a whole video, everything
    scopes = [scope_of(100), (10, 5), scope_of(2, 0, MS * (L - 2)), scope_of(3, MS * 100, MS * 180), scope_of(6), ALL]
    clips = R.clips_from(rows, "f16", [10, 20, 500, 870, 1600, 1999 - L], L, 9)
    for min_sep in (1, 8):
        got_r, _, _ = check(mem, clips, k, min_sep, "f16", scopes=scopes, label="mixed scopes")
        assert (got_r[:3] == -1).all()
        in3, in4 = got_r[3][got_r[3] >= 0], got_r[4][got_r[4] >= 0]
        assert ((in3 >= 850) & (in3 + L - 1 <= 930)).all() and got_r[3, 0] == 870
        assert ((in4 >= 1500) & (in4 + L - 1 < 1750)).all() and got_r[4, 0] == 1600
    check(mem, clips[:1], k, 8, "f16", scopes=scope_of(0), max_gap_ms=100, label="one pair for all")


def test_tags_sources_alternating_every_row():
    n = 600
    rows = R.scene_video(n, 128, "f16", 37)
    i = np.arange(n, dtype=np.int64)
    tags = ((i % 2) << 40) | (i * MS)
    mem = make_memory(rows, "f16", tags=tags)
    clips = R.clips_from(rows, "f16", [100, 300], 2, 1)
    got_r, got_s, _ = check(mem, clips, 5, 2, "f16", label="alternating")
    assert (got_r == -1).all() and (got_s == 0.0).all()
    check(mem, clips[:, :1].copy(), 5, 1, "f16", label="alternating L=1")   # single rows are still found


# ---- 5. ring ----------------------------------------------------------------------------------------------------------
def test_ring_windows_cross_the_physical_wrap():
    L = 16
    rows = R.scene_video(6000, 128, "f16", 41)
    mem = make_memory(rows, "f16", capacity=4096, ring=True, step=1000)
    base, host_rows = mem.rows_host()
    assert base == 1904 and host_rows.shape[0] == 4096
    # row id 4095 sits in the last physical slot, 4096 in slot 0; rows below 1904 were overwritten
    clips = R.clips_from(rows, "f16", [4088, 1896, 1904, 5984, 3000], L, 3)
    for min_sep in (1, 16):
        got_r, _, _ = check(mem, clips, 10, min_sep, "f16", label="ring")
        assert got_r[0, 0] == 4088 and got_r[2, 0] == 1904 and got_r[3, 0] == 5984
        live = got_r[got_r >= 0]
        assert (live >= 1904).all() and (live + L - 1 <= 5999).all()
    tagged = make_memory(rows, "f16", tags=contiguous_tags(6000, 6), capacity=4096, ring=True, step=1000)
    got_r, _, _ = check(tagged, clips, 10, 16, "f16", scopes=[ALL, ALL, scope_of(1), scope_of(5), scope_of(0)],
                        label="tagged ring")
    assert got_r[0, 0] == 4088 and (got_r[4] == -1).all()


# ---- 6. edges ---------------------------------------------------------------------------------------------------------
def test_fewer_rows_than_frames_and_exactly_one_window():
    from vidmem.memory import EmbeddingMemory
    rows = R.scene_video(200, 128, "f16", 43)
    clips = R.clips_from(rows, "f16", [0, 3], 8, 2)
    mem = EmbeddingMemory(128, 128, "f16")
    got_r, got_s, _ = check(mem, clips, 3, 8, "f16", label="n = 0")
    assert (got_r == -1).all()
    mem.append(from_bits(rows[:7], "f16"))
    got_r, got_s, _ = check(mem, clips, 3, 8, "f16", label="n < L")
    assert (got_r == -1).all() and (got_s == 0.0).all()
    mem.append(from_bits(rows[7:8], "f16"))
    got_r, _, _ = check(mem, clips, 3, 8, "f16", label="n == L")
    assert got_r[0].tolist() == [0, -1, -1]
    mem.append(from_bits(rows[8:100], "f16"))
    got_r, _, _ = check(mem, clips, 10, 32, "f16", label="fewer than k peaks")
    assert 0 < (got_r[0] >= 0).sum() < 10


def test_zero_frames_static_scene_and_min_score():
    n, L = 3000, 16
    rows = R.scene_video(n, 128, "f16", 45).copy()
    rows[1000:1040] = rows[1000]                        # a static scene of 40 identical rows
    mem = make_memory(rows, "f16")
    clips = R.clips_from(rows, "f16", [200, 1010, 2000, 2500], L, 4)
    clips[0, 5] = 0                                     # one zero frame: its term is an exact 0
    clips[2] = 0                                        # an all-zero clip: every window scores 0.0
    before = mem.clip_uncertified_count
    got_r, got_s, flags = check(mem, clips, 10, 16, "f16", label="edges")
    assert flags[0] == 0 and flags[3] == 0
    assert flags[1] != 0 and flags[2] != 0              # ties the fp32 stage cannot separate: redone, and still right
    assert got_r[1, 0] == 1000 and not ((got_r[1] > 1000) & (got_r[1] < 1040)).any()
    # every window ties at 0.0 and each but the first has an equal competitor at a lower start: one peak
    assert got_r[2].tolist() == [0] + [-1] * 9 and (got_s[2] == 0.0).all()
    assert mem.clip_uncertified_count == before + 2     # the counter accumulates over the fast calls
    check(mem, clips[3:], 10, 16, "f16")
    assert mem.clip_uncertified_count == before + 2
    check(mem, clips[1:2], 10, 16, "f16")
    assert mem.clip_uncertified_count == before + 3
    for mode, ms in ((0, 0.2), (1, 0.6), (0, -0.5), (1, 0.5), (0, 0.0)):
        check(mem, clips, 10, 16, "f16", min_score=ms, score_mode=mode, label=f"min_score {ms} mode {mode}")


def test_domain_row_outside_the_certificate_is_flagged_and_exact():
    n, L = 2000, 8
    bits = R.scene_video(n, 128, "bf16", 47)
    rows = from_bits(bits, "bf16")
    big, exact = domain_ref.scaled(rows[1234:1235], [50])            # norm 2^50: outside [2^-40, 2^40]
    assert exact
    rows[1234] = big[0]
    host = rows.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    mem = make_memory(host, "bf16")
    clips = R.clips_from(bits, "bf16", [1230, 400], L, 6)
    got_r, _, flags = check(mem, clips, 5, 8, "bf16", label="domain")
    assert (flags != 0).all() and got_r[0, 0] == 1230 and got_r[1, 0] == 400
    inside = make_memory(bits, "bf16")                              # the same rows without the plant: certified
    _, _, flags = check(inside, clips, 5, 8, "bf16", label="domain, no plant")
    assert (flags == 0).all()


# ---- 7. independence ----------------------------------------------------------------------------------------------------
def test_a_clip_alone_equals_the_clip_in_a_batch():
    rows, clips = parity_case(768, 16, 16, 10, "f16")
    mem = make_memory(rows, "f16")
    q = from_bits(clips, "f16")
    s5, r5 = mem.topk_clip(q, 10)
    for c in range(5):
        s1, r1 = mem.topk_clip(q[c:c + 1].contiguous(), 10)
        assert torch.equal(r1[0], r5[c]) and torch.equal(s1[0].view(torch.int64), s5[c].view(torch.int64))


# ---- 8. argument errors -------------------------------------------------------------------------------------------------
def raw_call(mem, clips, C_, L, k, min_sep, max_gap_ms=-1, scopes=None, ws_bytes=None, half_scope=False):
    """vm_topk_cosine_clip straight through ctypes -> (return code, scores, rows) with the outputs pre-filled."""
    from vidmem import _lib
    lib = mem.L
    need = int(lib.vm_topk_clip_workspace_bytes(mem.handle, 2, 8, 5))
    ws = torch.zeros(max(need, 256), dtype=torch.uint8, device="cuda")
    scores = torch.full((max(C_, 1) * max(k, 1),), 7.0, dtype=torch.float64, device="cuda")
    rows = torch.full((max(C_, 1) * max(k, 1),), 7, dtype=torch.int64, device="cuda")
    flags = torch.zeros(max(C_, 1), dtype=torch.int32, device="cuda")
    unc = torch.zeros(1, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    lo = hi = C.c_void_p(0)
    if scopes is not None:
        lo, hi = p(scopes[0]), (C.c_void_p(0) if half_scope else p(scopes[1]))
    rc = lib.vm_topk_cosine_clip(mem.handle, p(clips), C_, L, k, min_sep, max_gap_ms, lo, hi, 0, 0.0, 0, p(scores), p(rows),
                                 p(unc), p(flags), p(ws), need if ws_bytes is None else ws_bytes,
                                 _lib.current_stream_ptr())
    torch.cuda.synchronize()
    return rc, scores.cpu().numpy(), rows.cpu().numpy()


def test_argument_errors():
    from vidmem import _lib
    rows = R.scene_video(500, 128, "f16", 51)
    mem = make_memory(rows, "f16")
    tagged = make_memory(rows, "f16", tags=contiguous_tags(500, 2))
    clips = torch.zeros((2, 17, 128), dtype=torch.float16, device="cuda")
    assert raw_call(mem, clips, 2, 8, 5, 8)[0] == _lib.VM_OK
    for bad in (dict(L=0), dict(L=17), dict(min_sep=0), dict(min_sep=33), dict(k=0), dict(k=65), dict(C_=0)):
        a = dict(C_=2, L=8, k=5, min_sep=8)
        a.update(bad)
        rc, s, r = raw_call(mem, clips, **a)
        assert rc == _lib.VM_ERR_INVALID, bad
        assert (s == 7.0).all() and (r == 7).all()
    sc = torch.zeros((2, 2), dtype=torch.int64, device="cuda")
    assert raw_call(mem, clips, 2, 8, 5, 8, scopes=sc)[0] == _lib.VM_ERR_INVALID          # scopes, untagged memory
    assert raw_call(mem, clips, 2, 8, 5, 8, max_gap_ms=0)[0] == _lib.VM_ERR_INVALID       # max_gap_ms, untagged memory
    assert raw_call(tagged, clips, 2, 8, 5, 8, scopes=sc, half_scope=True)[0] == _lib.VM_ERR_INVALID
    assert raw_call(tagged, clips, 2, 8, 5, 8, scopes=sc, max_gap_ms=0)[0] == _lib.VM_OK
    need = int(mem.L.vm_topk_clip_workspace_bytes(mem.handle, 2, 8, 5))
    rc, s, r = raw_call(mem, clips, 2, 8, 5, 8, ws_bytes=need - 1)
    assert rc == _lib.VM_ERR_NOMEM and (s == 7.0).all() and (r == 7).all()            # refused before any launch
    for bad in ((2, 0, 5), (2, 17, 5), (0, 8, 5), (2, 8, 0), (2, 8, 65)):
        assert int(mem.L.vm_topk_clip_workspace_bytes(mem.handle, *bad)) == 0
    q = from_bits(R.clips_from(rows, "f16", [5], 8, 1), "f16")
    with pytest.raises(ValueError):
        mem.topk_clip(q, 5, scope=ALL)
    with pytest.raises(ValueError):
        mem.topk_clip(q, 5, max_gap_ms=10)
    with pytest.raises(ValueError):
        mem.topk_clip(q, 5, min_score=float("nan"))
    with pytest.raises(ValueError):
        mem.topk_clip(q, 5, min_sep=33)
    with pytest.raises(ValueError):
        mem.topk_clip(torch.zeros((1, 17, 128), device="cuda"), 5)
    s, r = mem.topk_clip(q[0], 5)                                                      # [L, D] is one clip
    assert r.shape == (1, 5) and r[0, 0] == 5


# ---- 9. graph capture -----------------------------------------------------------------------------------------------------
def test_graph_capture_append_and_clip_search_replayed():
    from vidmem.memory import EmbeddingMemory
    L, k, B, Cn = 8, 4, 128, 3
    bits = R.scene_video(1024, 128, "f16", 61)
    rows = from_bits(bits, "f16")
    mem = EmbeddingMemory(2048, 128, "f16", tagged=True)
    mem.append(rows[:256], tag=torch.arange(256, device="cuda") * MS)                # source 0
    scratch = mem.prepare_topk_clip(Cn, L, k)
    src = rows[256:256 + B].clone()
    tg = torch.zeros(B, dtype=torch.int64, device="cuda")
    q = torch.zeros((Cn, L, 128), dtype=torch.float16, device="cuda")
    scope = torch.zeros((Cn, 2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            mem.append(src, tag=tg)
            got_s, got_r = mem.enqueue_topk_clip(q, k, min_sep=4, scope=scope, max_gap_ms=100, scratch=scratch)
    torch.cuda.current_stream().wait_stream(s)
    mem.sync()                     # the capture advanced only the host mirror: back to the device count
    assert len(mem) == 256
    for rep in range(3):
        n_new = 256 + (rep + 1) * B
        src.copy_(rows[256 + rep * B:n_new])
        tg.copy_(((rep + 1) << 40) + torch.arange(B, device="cuda") * MS)
        starts = [n_new - L, 100, 252]                 # the newest rows; source 0; across the first boundary
        clips = R.clips_from(bits, "f16", starts, L, 70 + rep)
        q.copy_(from_bits(clips, "f16"))
        windows = [scope_of(rep + 1), scope_of(0, MS * 10, MS * 200), ALL]
        scope.copy_(torch.tensor(windows, dtype=torch.int64))
        graph.replay()
        torch.cuda.synchronize()
        assert mem.sync() == n_new
        base, host_rows = mem.rows_host()
        want_r, want_s = R.clip_topk(clips, host_rows, k, 4, "f16", tags=mem.tags_host(), scopes=windows, max_gap_ms=100,
                                     base=base)
        same(got_r.cpu().numpy(), got_s.cpu().numpy(), want_r, want_s, f"replay {rep}")
        assert want_r[0, 0] == n_new - L and want_r[1, 0] == 100 and 252 not in want_r[2]
