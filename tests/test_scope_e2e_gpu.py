"""GPU, end to end: ``memory.tag_by: time`` changes nothing the extractor writes; two clips share one memory, and the
retriever's vector leg and the pre-LLM similarity with a ``scope`` answer from the named clip or time window only - the
rows tests/scope_ref.py ranks first."""
import asyncio
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import scope_ref as S
from tests.search_checks import e2e_extractor
from tests.support import Embedder, bits

pytestmark = pytest.mark.gpu


def _extractor(enc, tag_by, look_ahead, group_by=None):
    return e2e_extractor(enc, {"tag_by": tag_by, "group_by": group_by}, look_ahead)


def _process(ex, clip, path, earlier=()):
    """``earlier``: the run ids of the clips this extractor has processed before (their rows are neighbours too)."""
    out = json.load(open(asyncio.run(ex.process_video(str(clip), str(path)))))
    rid = out["metadata"]["run_id"]
    names = {r: f"RUN{i}" for i, r in enumerate(list(earlier) + [rid])}

    def anon(i):
        return names.get(i.rsplit("_", 2)[0], "?") + "_" + "_".join(i.rsplit("_", 2)[1:]) if i else i
    res = [{**r, "processing_time": None, "group_time": None, "group_chunks": None,
            "similar": [[(anon(i), s) for i, s in fr] for fr in r["similar"]]}
           for r in out["results"]]
    out["metadata"].pop("run_id")
    out["metadata"]["config"]["memory"].pop("tag_by")
    return res, out["metadata"], rid


def _seconds(time_str):
    a, b = time_str.split("-")
    return tuple(int(x[:2]) * 60 + int(x[3:]) for x in (a, b))


@pytest.mark.parametrize("look_ahead", [1, 4])
def test_two_clips_one_tagged_memory(tmp_path, monkeypatch, look_ahead):
    from vidmem import _lib, specs, synthetic as syn
    from vidmem.memory import EmbeddingMemory, make_tag, scope_of
    from vidmem.similarity import HipPreLLMSimilarity, HipVectorSearch, batch_similarities
    monkeypatch.setitem(specs.SPECS, "vit_b16_2l", dict(specs.VIT_B16_224, layers=2))
    monkeypatch.chdir(tmp_path)
    clips = [tmp_path / "a.npy", tmp_path / "b.npy"]
    np.save(clips[0], syn.frames_u8(9, 240, 96, 128))             # 8 chunks of 30 frames at the default 30 fps
    np.save(clips[1], syn.frames_u8(10, 180, 96, 128))            # 6 chunks
    ex0 = _extractor(None, None, look_ahead)
    ex1 = _extractor(ex0.encoder, "time", look_ahead)
    assert not ex0.memory.tagged and ex1.memory.tagged and not ex1.memory.grouped
    rids0, rids = [], []
    for i, clip in enumerate(clips):
        res0, meta0, rid0 = _process(ex0, clip, tmp_path / f"plain_{i}.json", rids0)
        res1, meta1, rid = _process(ex1, clip, tmp_path / f"tagged_{i}.json", rids)
        assert res0 == res1 and meta0 == meta1
        assert any(i and i.startswith("RUN0") for r in res1 for fr in r["similar"] for i, _ in fr)
        rids0.append(rid0)
        rids.append(rid)
    assert torch.equal(ex0.memory.rows_tensor(), ex1.memory.rows_tensor())
    mem = ex1.memory
    n = len(mem)
    assert n == 70
    assert [mem.meta_of(r)["source"] for r in range(n)] == [0] * 40 + [1] * 30
    assert all("source" not in ex0.memory.meta_of(r) for r in range(n))
    tags = mem.tags_host()
    want_tags = [make_tag(0 if r < 40 else 1, ((r if r < 40 else r - 40) // 5) * 1000) for r in range(n)]
    assert tags.tolist() == want_tags

    # the vector leg: a question close to a frame of clip 0, asked of clip 1 only
    stored = mem.rows_tensor()
    noise = torch.randn(stored.shape[1], device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    q16 = (stored[7].float() + 0.02 * noise).to(torch.float16)
    emb = Embedder(q16.double().cpu().tolist())
    cfg = SimpleNamespace(top_k_chunks=6)
    vs = HipVectorSearch(mem, emb, cfg, min_score=-1.0, score_mode=_lib.VM_SCORE_RAW, scope=scope_of(1))
    got = asyncio.run(vs._vector_search_chunks(None, "q"))
    want_r, want_s = S.scoped_topk(bits(q16[None]), bits(stored), tags, scope_of(1), 6, min_score=-1.0)
    assert len(got) == 6 and all(c["id"].startswith(rids[1]) for c in got)
    assert [c["id"] for c in got] == [mem.id_of(int(r)) for r in want_r[0]]
    assert [c["score"] for c in got] == want_s[0].tolist()
    unscoped = HipVectorSearch(mem, emb, cfg, min_score=-1.0, score_mode=_lib.VM_SCORE_RAW)
    assert asyncio.run(unscoped._vector_search_chunks(None, "q"))[0]["id"] == mem.id_of(7)   # clip 0's frame wins unscoped

    # a time window of clip 0: seconds 2 to 4 (chunks starting at 2 s, 3 s and 4 s)
    win = scope_of(0, 2000, 4000)
    vs = HipVectorSearch(mem, emb, cfg, min_score=-1.0, score_mode=_lib.VM_SCORE_RAW, scope=win)
    got = asyncio.run(vs._vector_search_chunks(None, "q"))
    want_r, want_s = S.scoped_topk(bits(q16[None]), bits(stored), tags, win, 6, min_score=-1.0)
    assert [c["id"] for c in got] == [mem.id_of(int(r)) for r in want_r[0]]
    assert [c["score"] for c in got] == want_s[0].tolist()
    assert len(got) == 6 and all(c["id"].startswith(rids[0]) for c in got)
    assert all(2 <= _seconds(c["time"])[0] <= 4 for c in got) and {_seconds(c["time"])[0] for c in got} <= {2, 3, 4}

    # the pre-LLM similarity, scoped the same way; a wrong-length query lists the first in-scope rows
    sim = HipPreLLMSimilarity(mem, SimpleNamespace(top_k_chunk_with_batch_similarity=3), scope=scope_of(1))
    got = asyncio.run(sim._calculate_batch_similarities([q16, [0.0] * 5, stored[50]]))
    want_r, want_s = S.scoped_topk(bits(torch.stack([q16, stored[50]])), bits(stored), tags, scope_of(1), 3)
    assert [i for i, _ in got[0]] == [mem.id_of(int(r)) for r in want_r[0]]
    assert [s for _, s in got[0]] == want_s[0].tolist()
    assert [i for i, _ in got[2]] == [mem.id_of(int(r)) for r in want_r[1]] and got[2][0][0] == mem.id_of(50)
    assert got[1] == [(mem.id_of(40 + j), 0.0) for j in range(3)]
    assert batch_similarities(mem, [q16], 3, scope=scope_of(1)) == got[:1]

    # snapshot -> restore keeps tags and answers; an untagged memory's snapshot restores untagged
    mem.snapshot(str(tmp_path / "t.npz"))
    back = EmbeddingMemory.restore(str(tmp_path / "t.npz"))
    assert back.tagged and back.tags_host().tolist() == want_tags and back.new_source() == 2
    for a, b in zip(back.topk_scoped(q16[None], 5, win), mem.topk_scoped(q16[None], 5, win)):
        assert torch.equal(a, b)
    ex0.memory.snapshot(str(tmp_path / "p.npz"))
    old = EmbeddingMemory.restore(str(tmp_path / "p.npz"))
    assert not old.tagged
    with pytest.raises(ValueError, match="tagged"):
        old.topk_scoped(q16[None], 5, win)


def test_tag_by_time_with_group_by_chunk(tmp_path, monkeypatch):
    from vidmem import specs, synthetic as syn
    from vidmem.memory import scope_of
    monkeypatch.setitem(specs.SPECS, "vit_b16_2l", dict(specs.VIT_B16_224, layers=2))
    monkeypatch.chdir(tmp_path)
    clip = tmp_path / "a.npy"
    np.save(clip, syn.frames_u8(9, 120, 96, 128))
    ex = _extractor(None, "time", 4, group_by="chunk")
    assert ex.memory.tagged and ex.memory.grouped
    for i in range(2):
        _process(ex, clip, tmp_path / f"o{i}.json")
    mem = ex.memory
    assert len(mem) == 40 and len(set(mem.group_keys_host().tolist())) == 8
    q = mem.rows_tensor()[3:4].clone()
    _, r = mem.topk_scoped(q, 5, scope_of(1))
    assert (r[0] >= 20).all() and r[0, 0] == 23          # the same clip again: its copy in source 1
    _, r, _ = mem.topk_grouped(q, 3)
    assert r[0, 0] == 3
