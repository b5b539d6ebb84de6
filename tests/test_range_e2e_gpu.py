"""GPU, end to end: three videos in one tagged memory -> ``moments`` (range search + host segmentation) and
``similarity.frames_above`` against tests/range_ref.py."""
import numpy as np
import pytest
import torch

from tests import range_ref as R
from tests.support import bits

pytestmark = pytest.mark.gpu

D, RUNS, LEN, MS = 768, 6, 20, 33          # per video: 6 scenes of 20 near-identical frames, 33 ms apart
TAU, GAP = 0.5, 1000


def build(gap_inside=False):
    """Videos 0, 1, 2 appended one after the other; scene 3 of video 2 is also scene 1 of video 0 (the same place filmed
    twice).  ``gap_inside``: the second half of video 2's scene 3 is stamped 5 s later than it would be."""
    from vidmem.memory import EmbeddingMemory, make_tag
    g = torch.Generator(device="cuda").manual_seed(5)
    centres = torch.randn(3, RUNS, D, generator=g, device="cuda")
    centres[0, 1] = centres[2, 3]
    frames = centres[:, :, None, :] + 0.02 * torch.randn(3, RUNS, LEN, D, generator=g, device="cuda")
    frames = (frames / frames.norm(dim=-1, keepdim=True)).to(torch.float16)
    mem = EmbeddingMemory(3 * RUNS * LEN, D, "f16", tagged=True)
    for v in range(3):
        assert mem.new_source() == v
        ms = np.arange(RUNS * LEN, dtype=np.int64) * MS
        if gap_inside and v == 2:
            ms[3 * LEN + LEN // 2:] += 5000
        mem.append(frames[v].reshape(-1, D), ids=[f"v{v}_f{i}" for i in range(RUNS * LEN)],
                   tag=[make_tag(v, int(t)) for t in ms])
    query = (centres[2, 3] + 0.05 * torch.randn(D, generator=g, device="cuda")).to(torch.float16)[None].contiguous()
    return mem, query


def oracle(mem, query, scope):
    base, host = mem.rows_host()
    return R.range_hits(bits(query), host, TAU, tags=mem.tags_host(), scopes=scope, dtype="f16", base=base)[0]


def test_a_scene_comes_back_as_one_moment_of_its_video():
    from vidmem import _lib, similarity
    from vidmem.memory import scope_of
    mem, query = build()
    first = 2 * RUNS * LEN + 3 * LEN                       # row of the scene's first frame in video 2
    rows, scores, count = oracle(mem, query, scope_of(2))
    assert rows.tolist() == list(range(first, first + LEN)) and count == LEN       # the data does what it is meant to
    got = mem.moments(query, TAU, scope=scope_of(2), max_gap_ms=GAP)
    assert len(got) == 1 and len(got[0]) == 1
    m = got[0][0]
    peak = int(np.argmax(scores))
    assert (m.source, m.t0_ms, m.t1_ms) == (2, 3 * LEN * MS, (4 * LEN - 1) * MS)
    assert (m.first_row, m.last_row, m.hits) == (first, first + LEN - 1, LEN)
    assert m.peak_row == int(rows[peak])
    assert np.float64(m.peak_score).view(np.int64) == scores[peak].view(np.int64)
    # unscoped, the same place filmed in video 0 is a second moment
    both = mem.moments(query, TAU, max_gap_ms=GAP)[0]
    assert sorted((x.source, x.first_row, x.hits) for x in both) == [(0, LEN, LEN), (2, first, LEN)]
    assert both[0].peak_score >= both[1].peak_score
    # frames_above: the same rows as ids, in time order
    ids = similarity.frames_above(mem, query[0], TAU, score_mode=_lib.VM_SCORE_RAW, scope=scope_of(2))
    assert [i for i, _ in ids] == [f"v2_f{3 * LEN + j}" for j in range(LEN)]
    assert np.array_equal(np.array([s for _, s in ids]).view(np.int64), scores.view(np.int64))
    short = similarity.frames_above(mem, query[0].tolist(), TAU, score_mode=_lib.VM_SCORE_RAW, max_hits=3)
    assert [i for i, _ in short] == [f"v0_f{LEN + j}" for j in range(3)]
    with pytest.raises(ValueError, match="tagged"):
        from vidmem.memory import EmbeddingMemory
        EmbeddingMemory(16, D, "f16").moments(query, TAU)


def test_a_gap_wider_than_max_gap_ms_splits_the_scene():
    from vidmem.memory import scope_of
    mem, query = build(gap_inside=True)
    first = 2 * RUNS * LEN + 3 * LEN
    rows, scores, _ = oracle(mem, query, scope_of(2))
    assert rows.tolist() == list(range(first, first + LEN))
    got = mem.moments(query, TAU, scope=scope_of(2), max_gap_ms=GAP)[0]
    assert len(got) == 2
    halves = sorted(got, key=lambda x: x.first_row)
    assert (halves[0].first_row, halves[0].last_row) == (first, first + LEN // 2 - 1)
    assert (halves[1].first_row, halves[1].last_row) == (first + LEN // 2, first + LEN - 1)
    assert halves[1].t0_ms - halves[0].t1_ms == MS + 5000
    assert {got[0].peak_row, got[1].peak_row} == {int(rows[:LEN // 2][np.argmax(scores[:LEN // 2])]),
                                                  int(rows[LEN // 2:][np.argmax(scores[LEN // 2:])])}
    assert got[0].peak_score >= got[1].peak_score
    assert len(mem.moments(query, TAU, scope=scope_of(2), max_gap_ms=MS + 5000)[0]) == 1    # the gap itself still joins
