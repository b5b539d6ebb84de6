"""GPU, end to end: two clips through the extractor with ``memory.tag_by: time`` and ``memory.group_by: event`` share one
memory; the retriever's vector leg and the pre-LLM similarity with ``distinct=True`` and a ``scope`` then answer with one
frame per scene of the named clip only - the frames tests/group_scope_ref.py ranks first."""
import asyncio
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import cref
from tests import group_ref as G
from tests import group_scope_ref as GS
from tests.novelty_feed import threshold_between
from tests.search_checks import e2e_extractor, scene_clip
from tests.support import Embedder, bits

pytestmark = pytest.mark.gpu

LENGTHS = [[7, 3, 12, 1, 9, 8], [6, 2, 11, 4, 5, 2]]     # frames per scene of the two clips: 40 and 30 frames


def _process(ex, clip, path):
    return json.load(open(asyncio.run(ex.process_video(str(clip), str(path)))))["metadata"]["run_id"]


def test_one_frame_per_scene_of_one_video(tmp_path, monkeypatch):
    from vidmem import _lib, specs
    from vidmem.memory import scope_of
    from vidmem.similarity import HipPreLLMSimilarity, HipVectorSearch, batch_similarities
    monkeypatch.setitem(specs.SPECS, "vit_b16_2l", dict(specs.VIT_B16_224, layers=2))
    monkeypatch.chdir(tmp_path)
    clips, owner = [], []
    for i, lengths in enumerate(LENGTHS):
        frames, own = scene_clip(77 + i, lengths, 96, 128)
        clips.append(tmp_path / f"clip{i}.npz")
        np.savez(clips[i], frames=frames, fps=np.float64(5.0))      # 5 frames per one-second chunk: every frame is picked
        owner.append(own + (owner[-1][-1] + 1 if owner else 0))
    owner = np.concatenate(owner)
    ex0 = e2e_extractor(None, {})
    for i, clip in enumerate(clips):
        _process(ex0, clip, tmp_path / f"plain{i}.json")
    stored = ex0.memory.rows_host()[1]
    assert stored.shape[0] == owner.size == 70
    tau = threshold_between(cref.cosine_matrix(stored, stored), owner)          # from the reference's own scores
    ex = e2e_extractor(ex0.encoder, {"tag_by": "time", "group_by": "event", "event_threshold": tau})
    rids = [_process(ex, clip, tmp_path / f"event{i}.json") for i, clip in enumerate(clips)]
    mem = ex.memory
    assert mem.tagged and mem.grouped and np.array_equal(mem.rows_host()[1], stored)
    keys, tags = mem.group_keys_host(), mem.tags_host()
    assert np.array_equal(G.group_ids(keys), owner)                             # the events are the planted scenes
    assert [mem.meta_of(r)["source"] for r in range(70)] == [0] * 40 + [1] * 30

    # the vector leg: a question close to a frame of clip 0, asked for the scenes of clip 1 only
    rows = mem.rows_tensor()
    noise = torch.randn(rows.shape[1], device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    q16 = (rows[15].float() + 0.02 * noise).to(torch.float16)
    emb = Embedder(q16.double().cpu().tolist())
    cfg = SimpleNamespace(top_k_chunks=4)
    vs = HipVectorSearch(mem, emb, cfg, min_score=-1.0, score_mode=_lib.VM_SCORE_RAW, distinct=True, scope=scope_of(1))
    hits = asyncio.run(vs._vector_search_chunks(None, "q"))
    want_r, want_s, _ = GS.group_scoped_topk(bits(q16[None]), stored, keys, tags, scope_of(1), 4, min_score=-1.0)
    assert [c["id"] for c in hits] == [mem.id_of(int(r)) for r in want_r[0]]
    assert [c["score"] for c in hits] == want_s[0].tolist()
    assert len(hits) == 4 and all(c["id"].startswith(rids[1]) for c in hits)
    assert len({int(owner[int(r)]) for r in want_r[0]}) == 4                    # one frame per scene
    whole = HipVectorSearch(mem, emb, cfg, min_score=-1.0, score_mode=_lib.VM_SCORE_RAW, distinct=True)
    best = G.grouped_topk(bits(q16[None]), stored, keys, 1)[0][0, 0]           # without a scope clip 0's scene 2 wins
    assert asyncio.run(whole._vector_search_chunks(None, "q"))[0]["id"] == mem.id_of(int(best)) and owner[best] == 2

    # a window of clip 0 that cuts scene 2 (rows 10 .. 21) in two: seconds 3 to 5 are rows 15 .. 29
    win = scope_of(0, 3000, 5000)
    vs = HipVectorSearch(mem, emb, cfg, min_score=-1.0, score_mode=_lib.VM_SCORE_RAW, distinct=True, scope=win)
    hits = asyncio.run(vs._vector_search_chunks(None, "q"))
    want_r, want_s, _ = GS.group_scoped_topk(bits(q16[None]), stored, keys, tags, win, 4, min_score=-1.0)
    assert want_r[0, 3] == -1                      # three scenes have a frame in the window: the fourth hit is padding
    assert [c["id"] for c in hits] == [mem.id_of(int(r)) for r in want_r[0, :3]]
    assert [c["score"] for c in hits] == want_s[0, :3].tolist()
    assert sorted(int(owner[int(r)]) for r in want_r[0] if r >= 0) == [2, 3, 4] and ((want_r[0, :3] >= 15) & (want_r[0, :3] <= 29)).all()

    # the pre-LLM similarity, the same way; a wrong-length query lists the first in-scope row of the first in-scope scenes
    sims = batch_similarities(mem, [q16, [0.0] * 5, rows[50]], 3, distinct=True, scope=scope_of(1))
    want_r, want_s, _ = GS.group_scoped_topk(bits(torch.stack([q16, rows[50]])), stored, keys, tags, scope_of(1), 3)
    assert [i for i, _ in sims[0]] == [mem.id_of(int(r)) for r in want_r[0]]
    assert [s for _, s in sims[0]] == want_s[0].tolist()
    assert [i for i, _ in sims[2]] == [mem.id_of(int(r)) for r in want_r[1]] and sims[2][0][0] == mem.id_of(50)
    assert sims[1] == [(mem.id_of(r), 0.0) for r in (40, 46, 48)]
    pre = HipPreLLMSimilarity(mem, SimpleNamespace(top_k_chunk_with_batch_similarity=3), distinct=True, scope=scope_of(1))
    assert asyncio.run(pre._calculate_batch_similarities([q16])) == sims[:1]
