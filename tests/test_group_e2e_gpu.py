"""GPU, end to end: ``memory.group_by: chunk`` changes nothing the extractor writes, and the retriever's vector leg with
``distinct=True`` returns one hit per chunk - the chunks tests/group_ref.py ranks first."""
import asyncio
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import group_ref as G
from tests.search_checks import e2e_extractor
from tests.support import Embedder, bits

pytestmark = pytest.mark.gpu


def _run(tmp_path, clip, enc, group_by, look_ahead, tag):
    ex = e2e_extractor(enc, {"group_by": group_by}, look_ahead)
    out = json.load(open(asyncio.run(ex.process_video(str(clip), str(tmp_path / f"out_{tag}.json")))))
    rid = out["metadata"]["run_id"]
    res = [{**r, "processing_time": None, "group_time": None, "group_chunks": None,
            "similar": [[(i.replace(rid, "RUN") if i else i, s) for i, s in fr] for fr in r["similar"]]}
           for r in out["results"]]
    out["metadata"].pop("run_id")
    out["metadata"]["config"]["memory"].pop("group_by")
    return ex, res, out["metadata"], rid


@pytest.mark.parametrize("look_ahead", [1, 4])
def test_group_by_chunk_changes_no_output_and_search_is_distinct(tmp_path, monkeypatch, look_ahead):
    from vidmem import _lib, specs, synthetic as syn
    from vidmem.memory import EmbeddingMemory
    from vidmem.similarity import HipVectorSearch, batch_similarities
    monkeypatch.setitem(specs.SPECS, "vit_b16_2l", dict(specs.VIT_B16_224, layers=2))
    monkeypatch.chdir(tmp_path)
    clip = tmp_path / "clip.npy"
    np.save(clip, syn.frames_u8(9, 240, 96, 128))                 # 8 chunks of 30 frames at the default 30 fps
    ex0, res0, meta0, _ = _run(tmp_path, clip, None, None, look_ahead, "plain")
    ex1, res1, meta1, rid = _run(tmp_path, clip, ex0.encoder, "chunk", look_ahead, "grouped")
    assert not ex0.memory.grouped and ex1.memory.grouped
    assert res0 == res1 and meta0 == meta1
    assert torch.equal(ex0.memory.rows_tensor(), ex1.memory.rows_tensor())
    mem = ex1.memory
    n = len(mem)
    keys = mem.group_keys_host()
    batch = [mem.meta_of(r)["batch_id"] for r in range(n)]
    assert [batch[i] for i in range(n)] == [int(G.group_ids(keys)[i]) for i in range(n)]  # one group per chunk

    # the vector leg: a question close to one frame -> three distinct chunks, the best frame of each
    stored = mem.rows_tensor()
    noise = torch.randn(stored.shape[1], device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    q = stored[7].float() + 0.02 * noise
    q16 = q.to(torch.float16)
    vs = HipVectorSearch(mem, Embedder(q16.double().cpu().tolist()), SimpleNamespace(top_k_chunks=3),
                         min_score=-1.0, score_mode=_lib.VM_SCORE_RAW, distinct=True)
    got = asyncio.run(vs._vector_search_chunks(None, "q"))
    want_r, want_s, _ = G.grouped_topk(bits(q16[None]), bits(stored), keys, 3, min_score=-1.0)
    assert [c["id"] for c in got] == [mem.id_of(int(r)) for r in want_r[0]]
    assert [c["score"] for c in got] == want_s[0].tolist()
    got_batches = [int(c["id"].split("_")[-2]) for c in got]
    assert len(set(got_batches)) == 3 and got_batches == [batch[int(r)] for r in want_r[0]]
    sims = batch_similarities(mem, [q16], 3, distinct=True)
    assert [i for i, _ in sims[0]] == [c["id"] for c in got]

    # snapshot -> restore -> the same grouped answer; a plain memory's snapshot (no key field) restores plain
    mem.snapshot(str(tmp_path / "g.npz"))
    back = EmbeddingMemory.restore(str(tmp_path / "g.npz"))
    for a, b in zip(back.topk_grouped(q16[None], 5), mem.topk_grouped(q16[None], 5)):
        assert torch.equal(a, b)
    ex0.memory.snapshot(str(tmp_path / "p.npz"))
    old = EmbeddingMemory.restore(str(tmp_path / "p.npz"))
    assert not old.grouped and torch.equal(old.rows_tensor(), ex0.memory.rows_tensor())
    for a, b in zip(old.topk(q16[None], 5), ex0.memory.topk(q16[None], 5)):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="grouped"):
        old.topk_grouped(q16[None], 5)
