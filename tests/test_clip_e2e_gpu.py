"""GPU, end to end: ``similarity.clip_similarities`` - the reference's ``[(id, score), ...]`` list shape
(src/components/pre_llm_injector.py:346-372) over the clip search - against tests/clip_ref.py, and its result through
``merge_batch_similarities`` unchanged."""
import numpy as np
import pytest
import torch

from tests import clip_ref as R
from tests.search_checks import make_memory
from tests.support import MS, contiguous_tags, from_bits, scope_of

pytestmark = pytest.mark.gpu


def test_clip_similarities_ids_and_scores_match_the_oracle():
    from vidmem.similarity import clip_similarities, merge_batch_similarities
    n, D, k = 1500, 128, 4
    rows = R.scene_video(n, D, "f16", 71)
    tags = contiguous_tags(n, 3)
    mem = make_memory(rows[:0], "f16", tags=tags[:0], capacity=n)
    ids = [f"frame-{i}" for i in range(n)]
    mem.append(from_bits(rows, "f16"), ids=ids, tag=torch.as_tensor(tags).cuda())
    c16 = R.clips_from(rows, "f16", [100, 900], 16, 1)
    c5 = R.clips_from(rows, "f16", [640], 5, 2)
    vals16, vals5 = R.from_bits(c16, "f16"), R.from_bits(c5, "f16")
    # a tensor chunk, a failed embedding, a chunk of another length as lists, a second 16-frame chunk
    chunks = [torch.from_numpy(vals16[0]), RuntimeError("embedder failed"), vals5[0].tolist(), torch.from_numpy(vals16[1])]
    got = clip_similarities(mem, chunks, k)
    want16 = R.clip_topk(c16, rows, k, 16, "f16", tags=tags)
    want5 = R.clip_topk(c5, rows, k, 5, "f16", tags=tags)
    def listed(r, s):
        return [(ids[int(i)], float(x)) for i, x in zip(r, s) if i >= 0]
    assert got[0] == listed(want16[0][0], want16[1][0])
    assert got[1] == []
    assert got[2] == listed(want5[0][0], want5[1][0])
    assert got[3] == listed(want16[0][1], want16[1][1])
    assert got[0][0][0] == "frame-100" and got[2][0][0] == "frame-640" and got[3][0][0] == "frame-900"
    merged = merge_batch_similarities(got, 3)
    assert len(merged) == 3 and merged[0][1] == max(s for hits in got for _, s in hits)
    # one video only, with a clock rule
    sc = scope_of(1)
    got = clip_similarities(mem, [chunks[0], chunks[3]], k, min_sep=4, scope=sc, max_gap_ms=2 * MS)
    want = R.clip_topk(c16, rows, k, 4, "f16", tags=tags, scopes=sc, max_gap_ms=2 * MS)
    assert got[0] == listed(want[0][0], want[1][0]) and got[1] == listed(want[0][1], want[1][1])
    assert got[1][0][0] == "frame-900" and all(500 <= int(i.split("-")[1]) < 1000 for i, _ in got[0] + got[1])
    assert clip_similarities(mem, [], k) == [] and clip_similarities(mem, chunks, 0) == [[], [], [], []]
