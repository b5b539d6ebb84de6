"""GPU, end to end: ``memory.group_by: event`` changes nothing the extractor writes, leaves the memory's groups equal to
the events tests/events_ref.py finds in the stored rows - at look-ahead 1 and 4 alike - and the retriever's vector leg
with ``distinct=True`` then returns one frame per scene."""
import asyncio
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import cref
from tests import events_ref as E
from tests import group_ref as G
from tests.novelty_feed import threshold_between
from tests.search_checks import e2e_extractor, scene_clip
from tests.support import Embedder, bits

pytestmark = pytest.mark.gpu

LENGTHS = [7, 3, 12, 1, 9, 6, 2, 11, 4, 5]          # frames per scene: 60 frames, cuts inside and between chunks of 5


def _run(tmp_path, clip, enc, memory_cfg, look_ahead, tag):
    ex = e2e_extractor(enc, memory_cfg, look_ahead)
    out = json.load(open(asyncio.run(ex.process_video(str(clip), str(tmp_path / f"out_{tag}.json")))))
    rid = out["metadata"]["run_id"]
    res = [{**r, "processing_time": None, "group_time": None, "group_chunks": None,
            "similar": [[(i.replace(rid, "RUN") if i else i, s) for i, s in fr] for fr in r["similar"]]}
           for r in out["results"]]
    out["metadata"].pop("run_id")
    for key in ("group_by", "event_threshold"):           # the config echo
        out["metadata"]["config"]["memory"].pop(key)
    return ex, res, out["metadata"], rid


def test_group_by_event_changes_no_output_and_groups_are_the_scenes(tmp_path, monkeypatch):
    from vidmem import _lib, specs
    from vidmem.similarity import HipVectorSearch, batch_similarities
    monkeypatch.setitem(specs.SPECS, "vit_b16_2l", dict(specs.VIT_B16_224, layers=2))
    monkeypatch.chdir(tmp_path)
    frames, owner = scene_clip(77, LENGTHS, 96, 128)
    clip = tmp_path / "clip.npz"
    np.savez(clip, frames=frames, fps=np.float64(5.0))        # 5 frames per one-second chunk: every frame is picked
    ex0, res0, meta0, _ = _run(tmp_path, clip, None, {}, 1, "plain")
    stored = ex0.memory.rows_host()[1]
    n = stored.shape[0]
    assert n == sum(LENGTHS) and not ex0.memory.grouped
    tau = threshold_between(cref.cosine_matrix(stored, stored), owner)          # from the reference's own scores
    link = E.links(stored, "f16")
    flags = E.opens(link, tau)
    assert np.array_equal(flags, np.r_[True, owner[1:] != owner[:-1]])          # the events are the planted scenes
    want = E.regroup(flags)
    memories = []
    for look_ahead in (1, 4):
        if look_ahead != 1:             # the plain run at this look-ahead: the same results, its own config echo
            _, res_la, meta0, _ = _run(tmp_path, clip, ex0.encoder, {}, look_ahead, f"plain{look_ahead}")
            assert res_la == res0
        ex, res, meta, rid = _run(tmp_path, clip, ex0.encoder, {"group_by": "event", "event_threshold": tau},
                                  look_ahead, f"event{look_ahead}")
        assert ex.memory.grouped
        assert res == res0 and meta == meta0
        assert np.array_equal(ex.memory.rows_host()[1], stored)
        assert np.array_equal(ex.memory.group_keys_host(), want.keys), look_ahead
        memories.append((ex.memory, rid))
    mem, rid = memories[1]
    got = mem.events(tau)
    assert got.count == len(LENGTHS) and np.array_equal(got.first_rows.cpu().numpy(), want.keys[flags])

    # the vector leg: a question close to one frame -> distinct scenes, the best frame of each
    rows = mem.rows_tensor()
    noise = torch.randn(rows.shape[1], device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    q16 = (rows[15].float() + 0.02 * noise).to(torch.float16)
    vs = HipVectorSearch(mem, Embedder(q16.double().cpu().tolist()), SimpleNamespace(top_k_chunks=4),
                         min_score=-1.0, score_mode=_lib.VM_SCORE_RAW, distinct=True)
    hits = asyncio.run(vs._vector_search_chunks(None, "q"))
    want_r, want_s, _ = G.grouped_topk(bits(q16[None]), stored, want.keys, 4, min_score=-1.0)
    assert [c["id"] for c in hits] == [mem.id_of(int(r)) for r in want_r[0]]
    assert [c["score"] for c in hits] == want_s[0].tolist()
    scenes = [int(owner[int(r)]) for r in want_r[0]]
    assert len(set(scenes)) == 4 and scenes[0] == int(owner[15])               # one frame per scene
    sims = batch_similarities(mem, [q16], 4, distinct=True)
    assert [i for i, _ in sims[0]] == [c["id"] for c in hits]
