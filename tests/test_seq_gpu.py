"""GPU: the sequence search (vm_topk_cosine_seq, csrc/topk_seq.hip) against tests/seq_ref.py.

Bar: end rows, fp64 score bits, step rows, step score bits and padding identical to statement (A), for the fast and the
``exact=True`` entry on every case.  Data: the scene-structured "video" of tests/clip_ref.py; a sequence is J stored rows at
cumulative random gaps in 1 .. G plus 0.1 x unit noise (tests/seq_ref.steps_from).

Certified condition: the fast path must answer every sequence (flag 0) wherever a case says certified.  A case says so
only where ``seq_ref.margin`` - with the bit-exact oracle - is above 4 eps_seq(D, J) = 4 (cert_eps(D) + 2^-23) (the
certificate needs more than 2) and the best M end rows that could be possible peaks hold k exact peaks.  On the shapes used
here (margin in units of eps_seq; every one held k exact peaks):
  4,000 rows, C = 5   (D, J, G, min_sep, k, dtype): (768, 4, 4, 8, 10, f16) 12.4; (768, 16, 2, 16, 10, f16) 18.2;
                      (128, 3, 16, 32, 10, f16) 968; (768, 2, 16, 1, 10, f16) 42.9; (768, 5, 4, 16, 20, f16) 26.6;
                      (1024, 8, 3, 16, 10, bf16) 6.4
  20,000 rows x 128, J = 4, G = 8, min_sep = 16, C = 2: k = 1: 46,747; k = 3: 1,881
  70,000 rows x 128, J = 3, G = 4, min_sep = 8, C = 2: k = 1: 44,239; k = 3: 1,671
Every planted sequence is found first in every shape.  Run for parity alone, without the demand: (1024, 8, 3, 8, 20, bf16)
1.3 and (1024, 8, 3, 8, 20, f16) 1.2 - below the certificate's 2, and neither held k exact peaks among the best M - and
(768, 5, 4, 8, 20, f16) 5.3, which held them but stands too close to 4 for a demand.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import clip_ref as CL
from tests import domain_ref
from tests import mask_ref as MR
from tests import seq_ref as R
from tests.search_checks import make_memory
from tests.support import ALL, MS, check_entries, contiguous_tags, dev_mask, from_bits, scope_of

pytestmark = pytest.mark.gpu

# (D, J, G, min_sep, k, dtype) at 4,000 rows, C = 5
PARITY = [(768, 4, 4, 8, 10, "f16"), (768, 16, 2, 16, 10, "f16"), (128, 3, 16, 32, 10, "f16"), (768, 2, 16, 1, 10, "f16"),
          (768, 5, 4, 16, 20, "f16"), (1024, 8, 3, 16, 10, "bf16")]
UNCERTIFIED = [(1024, 8, 3, 8, 20, "bf16"), (1024, 8, 3, 8, 20, "f16"), (768, 5, 4, 8, 20, "f16")]
# (rows, D, J, G, min_sep): above the 16,384-slot cut sample; past one 65,536-row append
SIZES = [(20000, 128, 4, 8, 16), (70000, 128, 3, 4, 8)]


def parity_case(D, J, G, min_sep, k, dtype):
    rows = CL.scene_video(4000, D, dtype, 100 + D)
    steps, chains = R.steps_from(rows, dtype, R.pick_starts(4000, J, G, 5, J + G + min_sep), J, G, k)
    return rows, steps, chains


def size_case(n, D, J, G):
    rows = CL.scene_video(n, D, "f16", 200 + D)
    steps, chains = R.steps_from(rows, "f16", R.pick_starts(n, J, G, 2, n), J, G, 3)
    return rows, steps, chains


def check(mem, steps, k, G, min_sep, dtype, masks=None, index=None, max_gap_ms=None, min_score=None, score_mode=0,
          certified=None, want=None, label=""):
    """Fast and exact entry against statement (A) for the memory as it is.  masks: host uint32 [n_masks, W] or None.
    -> (rows, scores, step_rows, step_scores, flags) of the fast entry."""
    Cn = steps.shape[0]
    if want is None:
        base, host_rows = mem.rows_host()
        tags = mem.tags_host() if mem.tagged else None
        sel = None if masks is None else MR.selection(masks, index, Cn, base, host_rows.shape[0], mem.capacity)
        want = R.seq_topk(steps, host_rows, k, G, min_sep, dtype, tags=tags, sel=sel,
                          max_gap_ms=-1 if max_gap_ms is None else max_gap_ms, score_mode=score_mode, min_score=min_score,
                          base=base)
    m = None if masks is None else dev_mask(masks)
    q = from_bits(steps, dtype)

    def call(exact):
        s, r, sr, ss = mem.topk_seq(q, k, max_step=G, min_sep=min_sep, mask=m, mask_index=index, max_gap_ms=max_gap_ms,
                                    min_score=min_score, score_mode=score_mode, exact=exact)
        return r, s, sr, ss
    out = check_entries(call, lambda: mem.last_seq_flags[:Cn], want, certified, label)
    print(f"{label} k={k} C={Cn} flagged={int((out[-1] != 0).sum())}")
    return out


# ---- 1. identities --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [128, 768])
def test_one_step_equals_topk_and_topk_masked(D):
    rows = CL.scene_video(4000, D, "f16", 100 + D)
    mem = make_memory(rows, "f16")
    steps, _ = R.steps_from(rows, "f16", R.pick_starts(4000, 1, 1, 5, 1), 1, 1, 2)
    q = from_bits(steps, "f16")
    masks = np.random.default_rng(D).integers(0, 1 << 32, (2, mem.mask_words), dtype=np.uint64).astype(np.uint32)
    index = [0, 1, 1, 0, 7]                               # 7: out of range = the empty mask
    s0, r0 = mem.topk(q[:, 0].contiguous(), 10)
    sm, rm = mem.topk_masked(q[:, 0].contiguous(), 10, dev_mask(masks), mask_index=index)
    for exact in (False, True):
        s1, r1, sr, ss = mem.topk_seq(q, 10, max_step=3, min_sep=1, exact=exact)
        assert torch.equal(r1, r0) and torch.equal(s1.view(torch.int64), s0.view(torch.int64)), exact
        assert torch.equal(sr[:, :, 0], r1) and torch.equal(ss[:, :, 0].view(torch.int64), s1.view(torch.int64))
        s2, r2, _, _ = mem.topk_seq(q, 10, max_step=3, min_sep=1, mask=dev_mask(masks), mask_index=index, exact=exact)
        assert torch.equal(r2, rm) and torch.equal(s2.view(torch.int64), sm.view(torch.int64)), exact
        assert (r2[4] == -1).all()
    check(mem, steps, 10, 3, 1, "f16", label="J=1")


def test_max_step_1_equals_topk_clip_with_tags_gap_and_scope():
    n, J = 2000, 8
    rows = CL.scene_video(n, 128, "f16", 31)
    tags = contiguous_tags(n, 8)
    i = np.arange(n)
    tags[(i % 250) > 100] += 5000
    mem = make_memory(rows, "f16", tags=tags)
    clips = CL.clips_from(rows, "f16", [246, 700, 1493, 96, 1984], J, 5)
    q = from_bits(clips, "f16")
    scopes = [scope_of(0), scope_of(2), scope_of(5, 0, MS * 200), (10, 5), ALL]
    masks = torch.stack([mem.mask_of_scope(sc) for sc in scopes])
    for min_sep, gap, mode, ms in ((8, None, 0, None), (1, 1000, 1, 0.55), (16, 0, 0, None)):
        for exact in (False, True):
            s0, r0 = mem.topk_clip(q, 6, min_sep=min_sep, max_gap_ms=gap, min_score=ms, score_mode=mode)
            s1, r1, sr, _ = mem.topk_seq(q, 6, max_step=1, min_sep=min_sep, max_gap_ms=gap, min_score=ms, score_mode=mode,
                                         exact=exact)
            want_r = torch.where(r0 >= 0, r0 + J - 1, r0)
            assert torch.equal(r1, want_r) and torch.equal(s1.view(torch.int64), s0.view(torch.int64)), (min_sep, exact)
            assert torch.equal(sr[:, :, 0][r1 >= 0], r0[r0 >= 0])
            s0, r0 = mem.topk_clip(q, 6, min_sep=min_sep, scope=scopes, max_gap_ms=gap, min_score=ms, score_mode=mode)
            s1, r1, _, _ = mem.topk_seq(q, 6, max_step=1, min_sep=min_sep, mask=masks, max_gap_ms=gap, min_score=ms,
                                        score_mode=mode, exact=exact)
            want_r = torch.where(r0 >= 0, r0 + J - 1, r0)
            assert torch.equal(r1, want_r) and torch.equal(s1.view(torch.int64), s0.view(torch.int64)), (min_sep, exact)
            # max_gap_ms = 0 leaves no two adjacent rows joined: only then is every sequence without an END
            assert (r1[3] == -1).all() and bool((r1[0] >= 0).any()) == (gap != 0)


# ---- 2. parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,J,G,min_sep,k,dtype", PARITY)
def test_parity_certified(D, J, G, min_sep, k, dtype):
    rows, steps, chains = parity_case(D, J, G, min_sep, k, dtype)
    mem = make_memory(rows, dtype)
    got = check(mem, steps, k, G, min_sep, dtype, certified=True, label=f"parity {dtype} D={D} J={J} G={G} sep={min_sep}")
    got_r, step_rows = got[0], got[2]
    for c in range(5):
        assert abs(int(got_r[c, 0]) - int(chains[c, -1])) < max(min_sep, 2)      # the sequence finds its own moment
        live = np.sort(got_r[c][got_r[c] >= 0])
        assert (np.diff(live) >= min_sep).all()
        d = np.diff(step_rows[c][got_r[c] >= 0], axis=1)
        assert ((d >= 1) & (d <= G)).all()


@pytest.mark.parametrize("D,J,G,min_sep,k,dtype", UNCERTIFIED)
def test_parity_without_the_flag_demand(D, J, G, min_sep, k, dtype):
    rows, steps, _ = parity_case(D, J, G, min_sep, k, dtype)
    check(make_memory(rows, dtype), steps, k, G, min_sep, dtype, label=f"parity {dtype} D={D} J={J} G={G} sep={min_sep}")


# ---- 3. selection at size -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,J,G,min_sep", SIZES)
def test_selection_at_size_certified(n, D, J, G, min_sep):
    rows, steps, chains = size_case(n, D, J, G)
    mem = make_memory(rows, "f16")
    want = R.seq_topk(steps, rows, 3, G, min_sep, "f16")
    got = check(mem, steps, 3, G, min_sep, "f16", certified=True, want=want, label=f"size {n}")
    assert [abs(int(got[0][c, 0]) - int(chains[c, -1])) < min_sep for c in range(2)] == [True, True]
    # without a filter the k = 1 answer is the first column of the k = 3 answer (one ranking of the peaks)
    check(mem, steps, 1, G, min_sep, "f16", certified=True, want=tuple(w[:, :1] for w in want), label=f"size {n}")


# ---- 4. the align kernel's seams ------------------------------------------------------------------------------------
def test_longest_span_and_chains_across_every_segment_seam():
    n, J, G = 4000, 16, 16
    rows = CL.scene_video(n, 128, "f16", 71)
    seams = list(range(R.SEQ_SEG, n, R.SEQ_SEG))
    assert len(seams) == 5
    # span 241: the chain that ends ON the first row of a segment reaches 240 rows back; one chain straddles every seam
    full = np.stack([s - 16 * np.arange(J)[::-1] for s in seams[:2]])
    steps = R.steps_at(rows, "f16", full, 3)
    mem = make_memory(rows, "f16")
    got = check(mem, steps, 4, G, 32, "f16", label="span 241")
    for c in range(2):
        assert got[0][c, 0] == seams[c] and np.array_equal(got[2][c, 0], full[c])
    J, G = 6, 7
    starts = [s - 17 for s in seams] + [0, n - 1 - 5 * 7]
    chains = np.stack([s + 7 * np.arange(J) for s in starts])      # every step the longest allowed
    assert all(chains[i, 0] < s < chains[i, -1] for i, s in enumerate(seams))
    assert chains[5, 0] == 0 and chains[6, -1] == n - 1
    steps = R.steps_at(rows, "f16", chains, 4)
    got = check(mem, steps, 4, G, 16, "f16", label="seams")
    for c in range(7):
        assert got[0][c, 0] == chains[c, -1] and np.array_equal(got[2][c, 0], chains[c]), c


def test_ring_chains_cross_the_physical_wrap_and_stop_at_the_oldest_row():
    J, G = 6, 5
    rows = CL.scene_video(6000, 128, "f16", 41)
    mem = make_memory(rows, "f16", capacity=4096, ring=True, step=1000)
    base, host_rows = mem.rows_host()
    assert base == 1904 and host_rows.shape[0] == 4096
    # row id 4095 sits in the last physical slot, 4096 in slot 0; rows below 1904 were overwritten
    chains = np.stack([4085 + 4 * np.arange(J), 1896 + 5 * np.arange(J), 1904 + 3 * np.arange(J),
                       5999 - 5 * np.arange(J)[::-1]])
    steps = R.steps_at(rows, "f16", chains, 5)
    for min_sep in (1, 16):
        got = check(mem, steps, 8, G, min_sep, "f16", label="ring")
        assert got[0][0, 0] == chains[0, -1] and np.array_equal(got[2][0, 0], chains[0])
        assert got[0][2, 0] == chains[2, -1] and got[0][3, 0] == 5999
        live = got[2][got[2] >= 0]
        assert (live >= 1904).all() and (live <= 5999).all()
    # the chain planted from row 1896 lost its first two rows: what is left of it cannot be the answer as planted
    assert not np.array_equal(got[2][1, 0], chains[1])
    tagged = make_memory(rows, "f16", tags=contiguous_tags(6000, 6), capacity=4096, ring=True, step=1000)
    check(tagged, steps, 8, G, 16, "f16", label="tagged ring")


# ---- 5. tags --------------------------------------------------------------------------------------------------------
def test_tags_no_chain_spans_two_videos():
    n, J, G = 2000, 5, 4
    rows = CL.scene_video(n, 128, "f16", 31)
    tags = contiguous_tags(n, 8)                        # 8 sources of 250 rows
    mem = make_memory(rows, "f16", tags=tags, grouped=True)
    chains = np.stack([s + 3 * np.arange(J) for s in (244, 700, 1494, 30, 1980)])   # 244, 1494: planted across a boundary
    steps = R.steps_at(rows, "f16", chains, 5)
    for min_sep in (1, 16):
        got = check(mem, steps, 10, G, min_sep, "f16", label="sources")
        sr = got[2]
        live = sr[:, :, 0] >= 0
        assert ((sr[:, :, 0][live] // 250) == (sr[:, :, -1][live] // 250)).all()
        assert not np.array_equal(sr[0, 0], chains[0]) and not np.array_equal(sr[2, 0], chains[2])
        assert np.array_equal(sr[1, 0], chains[1])
    plain = make_memory(rows, "f16")                    # the untagged twin does return the straddling chains
    got = check(plain, steps, 10, G, 16, "f16", label="untagged twin")
    assert np.array_equal(got[2][0, 0], chains[0]) and np.array_equal(got[2][2, 0], chains[2])


def test_tags_sources_alternating_every_row():
    n = 600
    rows = CL.scene_video(n, 128, "f16", 37)
    i = np.arange(n, dtype=np.int64)
    mem = make_memory(rows, "f16", tags=((i % 2) << 40) | (i * MS))
    steps, _ = R.steps_from(rows, "f16", [100, 300], 2, 3, 1)
    got = check(mem, steps, 5, 3, 2, "f16", label="alternating")
    assert (got[0] == -1).all() and (got[1] == 0.0).all() and (got[2] == -1).all()
    got = check(mem, steps[:, :1].copy(), 5, 3, 1, "f16", label="alternating J=1")   # single rows are still found
    assert (got[0] >= 0).all()


def test_tags_max_gap_cuts_a_chain_and_untimed_rows():
    n, J, G = 1500, 4, 3
    rows = CL.scene_video(n, 128, "f16", 33)
    tags = contiguous_tags(n, 3)
    i = np.arange(n)
    tags[(i % 500) > 100] += 5000                       # a 5 s jump after row 100 of every source
    tags[(i % 500) > 300] -= 2000                       # the clock runs backwards after row 300
    tags[40:44] = CL.INT64_MIN                          # untimed rows: a chain may lie inside them, not across their ends
    tags[900] = CL.INT64_MIN
    mem = make_memory(rows, "f16", tags=tags)
    chains = np.stack([s + 2 * np.arange(J) for s in (97, 297, 36, 40, 896, 1200)])
    chains[3] = [40, 41, 42, 43]
    steps = R.steps_at(rows, "f16", chains, 7)
    for gap in (None, 1000, 0):
        check(mem, steps, 8, G, 8, "f16", max_gap_ms=gap, label=f"max_gap_ms={gap}")
    got = check(mem, steps, 8, G, 8, "f16", max_gap_ms=1000)
    assert not np.array_equal(got[2][0, 0], chains[0]) and not np.array_equal(got[2][1, 0], chains[1])
    got = check(mem, steps, 8, G, 8, "f16")
    assert np.array_equal(got[2][0, 0], chains[0]) and np.array_equal(got[2][1, 0], chains[1])
    assert not np.array_equal(got[2][2, 0], chains[2]) and np.array_equal(got[2][3, 0], chains[3])
    assert not np.array_equal(got[2][4, 0], chains[4])  # row 900 is stepped OVER by the planted chain: still a break


# ---- 6. masks -------------------------------------------------------------------------------------------------------
def test_masks_stepped_over_rows_empty_mask_and_per_sequence_masks():
    n, J = 2000, 4
    rows = CL.scene_video(n, 128, "f16", 53)
    mem = make_memory(rows, "f16", capacity=2048)
    W = mem.mask_words
    even = np.full(W, 0x55555555, np.uint32)
    chains = np.stack([s + 2 * np.arange(J) for s in (100, 901, 1500)])
    steps = R.steps_at(rows, "f16", chains, 9)
    got = check(mem, steps, 6, 2, 4, "f16", masks=even[None], label="every second row")
    assert np.array_equal(got[2][0, 0], chains[0]) and np.array_equal(got[2][2, 0], chains[2])
    assert (got[2][got[2] >= 0] % 2 == 0).all()         # chains step over the odd rows; 901 .. 907 is not selected
    got = check(mem, steps, 6, 1, 4, "f16", masks=even[None], label="every second row, G=1")
    assert (got[0] == -1).all()                         # no two selected rows are adjacent
    got = check(mem, steps[:, :1].copy(), 6, 1, 1, "f16", masks=even[None], label="every second row, J=1")
    assert (got[0] >= 0).all()
    empty = np.zeros(W, np.uint32)
    got = check(mem, steps, 6, 2, 4, "f16", masks=empty[None], label="empty mask")
    assert (got[0] == -1).all() and (got[1] == 0.0).all() and (got[2] == -1).all() and (got[3] == 0.0).all()
    got = check(mem, steps, 6, 2, 4, "f16", masks=np.stack([even, ~even]), index=[0, 5, -1], label="index out of range")
    assert (got[0][1:] == -1).all() and (got[0][0] >= 0).any()
    three = np.stack([even, ~even, MR.pack_rows(range(1400, 1600), mem.capacity)])
    got = check(mem, steps, 6, 2, 4, "f16", masks=three, label="one mask per sequence")
    assert np.array_equal(got[2][1, 0], chains[1]) and np.array_equal(got[2][2, 0], chains[2])
    got = check(mem, steps, 6, 2, 4, "f16", masks=three, index=[2, 2, 0], label="indexed masks")
    assert (got[2][0][got[2][0] >= 0] >= 1400).all()


# ---- 7. degenerate inputs -------------------------------------------------------------------------------------------
def test_fewer_rows_than_steps_and_exactly_one_chain():
    from vidmem.memory import EmbeddingMemory
    rows = CL.scene_video(200, 128, "f16", 43)
    steps, _ = R.steps_from(rows, "f16", [0, 3], 8, 1, 2)
    mem = EmbeddingMemory(128, 128, "f16")
    got = check(mem, steps, 3, 2, 8, "f16", label="n = 0")
    assert (got[0] == -1).all()
    mem.append(from_bits(rows[:7], "f16"))
    got = check(mem, steps, 3, 2, 8, "f16", label="n < J")
    assert (got[0] == -1).all() and (got[1] == 0.0).all()
    mem.append(from_bits(rows[7:8], "f16"))
    got = check(mem, steps, 3, 2, 8, "f16", label="n == J")
    assert got[0][0].tolist() == [7, -1, -1] and got[2][0, 0].tolist() == list(range(8))
    mem.append(from_bits(rows[8:100], "f16"))
    got = check(mem, steps, 10, 2, 32, "f16", label="fewer than k peaks")
    assert 0 < (got[0][0] >= 0).sum() < 10


def test_zero_steps_static_scene_score_modes_and_min_score():
    n, J, G = 3000, 6, 3
    rows = CL.scene_video(n, 128, "f16", 45).copy()
    rows[1000:1200] = rows[1000]                        # a static scene of 200 identical rows
    mem = make_memory(rows, "f16")
    steps, chains = R.steps_from(rows, "f16", [200, 1050, 2000, 2500], J, G, 4)
    steps[0, 3] = 0                                     # one zero step: its term is an exact 0
    steps[2] = 0                                        # an all-zero sequence: every chain scores 0.0
    before = mem.seq_uncertified_count
    got = check(mem, steps, 10, G, 16, "f16", label="edges")
    got_r, got_s, got_sr, _, flags = got
    assert flags[0] == 0 and flags[3] == 0
    assert flags[1] != 0 and flags[2] != 0              # ties the fp32 stage cannot separate: redone, and still right
    # inside the static scene every predecessor ties: the chain takes the NEAREST row at every step, and of the tied end
    # rows the lowest is the peak
    inside = (got_sr[1, :, 0] >= 1000) & (got_sr[1, :, -1] < 1200)
    assert inside.any() and (np.diff(got_sr[1][inside], axis=1) == 1).all()
    # every chain ties at 0.0 and each end row but the first has an equal competitor at a lower row: one peak
    assert got_r[2].tolist() == [J - 1] + [-1] * 9 and (got_s[2] == 0.0).all()
    assert got_sr[2, 0].tolist() == list(range(J))
    assert mem.seq_uncertified_count == before + 2      # the counter accumulates over the fast calls
    for mode, ms in ((0, 0.2), (1, 0.6), (0, -0.5), (1, 0.5), (0, 0.0)):
        check(mem, steps, 10, G, 16, "f16", min_score=ms, score_mode=mode, label=f"min_score {ms} mode {mode}")


def test_domain_row_outside_the_certificate_is_flagged_and_exact():
    n, J, G = 2000, 4, 3
    bits = CL.scene_video(n, 128, "bf16", 47)
    rows = from_bits(bits, "bf16")
    big, exact = domain_ref.scaled(rows[1234:1235], [50])            # norm 2^50: outside [2^-40, 2^40]
    assert exact
    rows[1234] = big[0]
    host = rows.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    mem = make_memory(host, "bf16")
    steps, chains = R.steps_from(bits, "bf16", [1230, 400], J, G, 6)
    got = check(mem, steps, 5, G, 8, "bf16", label="domain")
    assert (got[-1] != 0).all() and got[0][1, 0] == chains[1, -1]
    inside = make_memory(bits, "bf16")                              # the same rows without the plant: certified
    got = check(inside, steps, 5, G, 8, "bf16", label="domain, no plant")
    assert (got[-1] == 0).all()


# ---- 8. independence ------------------------------------------------------------------------------------------------
def test_a_sequence_alone_equals_the_sequence_in_a_batch():
    rows, steps, _ = parity_case(768, 4, 4, 8, 10, "f16")
    mem = make_memory(rows, "f16")
    q = from_bits(steps, "f16")
    five = mem.topk_seq(q, 10, max_step=4, min_sep=8)
    for c in range(5):
        one = mem.topk_seq(q[c:c + 1].contiguous(), 10, max_step=4, min_sep=8)
        for a, b in zip(one, five):
            assert torch.equal(a[0].view(torch.int64) if a.dtype == torch.float64 else a[0],
                               b[c].view(torch.int64) if b.dtype == torch.float64 else b[c])


# ---- 9. argument errors ---------------------------------------------------------------------------------------------
def raw_call(mem, steps, C_=2, J=4, k=5, G=3, min_sep=8, max_gap_ms=-1, masks=None, n_masks=0, index=None, use_min=0,
             min_score=0.0, ws_bytes=None, ws_shift=0, null=(), exact=False):
    """vm_topk_cosine_seq straight through ctypes -> (return code, every output) with the outputs pre-filled."""
    from vidmem import _lib
    lib = mem.L
    need = int(lib.vm_topk_seq_workspace_bytes(mem.handle, 2, 4, 5))
    ws = torch.zeros(max(need, 256) + 256, dtype=torch.uint8, device="cuda")
    n = max(C_, 1) * max(k, 1)
    outs = dict(scores=torch.full((n,), 7.0, dtype=torch.float64, device="cuda"),
                rows=torch.full((n,), 7, dtype=torch.int64, device="cuda"),
                step_rows=torch.full((n * 16,), 7, dtype=torch.int64, device="cuda"),
                step_scores=torch.full((n * 16,), 7.0, dtype=torch.float64, device="cuda"))
    flags = torch.zeros(max(C_, 1), dtype=torch.int32, device="cuda")
    unc = torch.zeros(1, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    o = {name: (None if name in null else t) for name, t in outs.items()}
    head = (mem.handle, p(None if "steps" in null else steps), C_, J, k, G, min_sep, max_gap_ms, p(masks), n_masks,
            p(index), use_min, min_score, 0, p(o["scores"]), p(o["rows"]), p(o["step_rows"]), p(o["step_scores"]))
    tail = (C.c_void_p(ws.data_ptr() + ws_shift), need if ws_bytes is None else ws_bytes, _lib.current_stream_ptr())
    if exact:
        rc = lib.vm_topk_cosine_seq_exact(*head, *tail)
    else:
        rc = lib.vm_topk_cosine_seq(*head, p(unc), p(flags), *tail)
    torch.cuda.synchronize()
    return rc, [t.cpu().numpy() for t in outs.values()]


def test_argument_errors_leave_the_outputs_untouched():
    from vidmem import _lib
    rows = CL.scene_video(500, 128, "f16", 51)
    mem = make_memory(rows, "f16")
    tagged = make_memory(rows, "f16", tags=contiguous_tags(500, 2))
    steps = torch.zeros((2, 17, 128), dtype=torch.float16, device="cuda")
    masks = torch.zeros((3, mem.mask_words), dtype=torch.int32, device="cuda")
    idx = torch.zeros(2, dtype=torch.int32, device="cuda")

    def untouched(outs):
        return all((o == 7).all() for o in outs)
    for exact in (False, True):
        assert raw_call(mem, steps, exact=exact)[0] == _lib.VM_OK
        assert raw_call(mem, steps, null=("step_rows", "step_scores"), exact=exact)[0] == _lib.VM_OK
        assert raw_call(mem, steps, masks=masks, n_masks=3, index=idx, exact=exact)[0] == _lib.VM_OK
        assert raw_call(tagged, steps, max_gap_ms=0, exact=exact)[0] == _lib.VM_OK
        bad = [dict(J=0), dict(J=17), dict(G=0), dict(G=17), dict(min_sep=0), dict(min_sep=33), dict(k=0), dict(k=65),
               dict(C_=0), dict(null=("steps",)), dict(null=("scores",)), dict(null=("rows",)),
               dict(use_min=1, min_score=float("nan")), dict(max_gap_ms=0),
               dict(masks=masks, n_masks=3), dict(masks=masks, n_masks=0, index=idx), dict(ws_shift=128)]
        for a in bad:
            rc, outs = raw_call(mem, steps, exact=exact, **a)
            assert rc == _lib.VM_ERR_INVALID and untouched(outs), (a, rc)
            assert mem.L.vm_last_error(mem.ctx.handle), a
        rc, outs = raw_call(mem, steps.view(-1)[1:], exact=exact)                    # steps 2 bytes off a 16-byte boundary
        assert rc == _lib.VM_ERR_INVALID and untouched(outs)
        rc, outs = raw_call(mem, steps, masks=masks, n_masks=1 << 27, index=idx, exact=exact)   # 2^31 words of masks
        assert rc == _lib.VM_ERR_UNSUPPORTED and untouched(outs)
        need = int(mem.L.vm_topk_seq_workspace_bytes(mem.handle, 2, 4, 5))
        rc, outs = raw_call(mem, steps, ws_bytes=need - 1, exact=exact)
        assert rc == _lib.VM_ERR_NOMEM and untouched(outs)                          # refused before any launch
    for bad in ((2, 0, 5), (2, 17, 5), (0, 8, 5), (2, 8, 0), (2, 8, 65)):
        assert int(mem.L.vm_topk_seq_workspace_bytes(mem.handle, *bad)) == 0
    q = from_bits(R.steps_from(rows, "f16", [5], 4, 2, 1)[0], "f16")
    for kw in (dict(max_gap_ms=10), dict(min_score=float("nan")), dict(min_sep=33), dict(max_step=0), dict(max_step=17),
               dict(mask_index=[0]), dict(mask=torch.zeros(3, dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError):
            mem.topk_seq(q, 5, **kw)
    with pytest.raises(ValueError):
        mem.topk_seq(torch.zeros((1, 17, 128), device="cuda"), 5)
    s, r, sr, ss = mem.topk_seq(q[0], 5, max_step=2)                                  # [J, D] is one sequence
    assert r.shape == (1, 5) and sr.shape == (1, 5, 4) and sr[0, 0, 0] == 5
