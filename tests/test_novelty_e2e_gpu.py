"""GPU, end to end: the extractor with ``memory.novelty_threshold`` on a clip whose frames repeat - look-ahead 1 and 4
give identical output and memories, the output says which row stands for every frame, and a snapshot of the gated
memory restores to one that answers alike."""
import asyncio
import json

import numpy as np
import pytest
import torch

from oracle import cref
from tests import novelty_ref as N
from tests.novelty_feed import feed, threshold_between
from tests.search_checks import e2e_extractor
from tests.support import bits

pytestmark = pytest.mark.gpu


def _process(ex, clip, path):
    out = json.load(open(asyncio.run(ex.process_video(str(clip), str(path)))))
    rid = out["metadata"]["run_id"]
    anon = lambda i: i.replace(rid, "RUN") if i else i
    res = [{**r, "processing_time": None, "group_time": None, "group_chunks": None,
            "similar": [[(anon(i), s) for i, s in fr] for fr in r["similar"]]} for r in out["results"]]
    return res, rid


def test_gated_extractor_look_ahead_1_and_4_alike(tmp_path, monkeypatch):
    from vidmem import specs
    from vidmem.memory import EmbeddingMemory
    monkeypatch.setitem(specs.SPECS, "vit_b16_2l", dict(specs.VIT_B16_224, layers=2))
    monkeypatch.chdir(tmp_path)
    frames, owner = feed(77, 50, 96, 128, block=16)
    frames, owner = frames[:120], owner[:120]
    clip = tmp_path / "clip.npz"
    np.savez(clip, frames=frames, fps=np.float64(5.0))        # 5 frames per one-second chunk: every frame is picked
    ex_off = e2e_extractor(None, {"novelty_threshold": None}, 1)
    enc = ex_off.encoder
    all_emb = enc.embed_frames(torch.from_numpy(frames).cuda())
    emb_bits = bits(all_emb)
    tau = threshold_between(cref.cosine_matrix(emb_bits, emb_bits), owner)
    ex1, ex4 = (e2e_extractor(enc, {"novelty_threshold": tau}, la) for la in (1, 4))
    res1, rid1 = _process(ex1, clip, tmp_path / "la1.json")
    res4, rid4 = _process(ex4, clip, tmp_path / "la4.json")
    assert res1 == res4 and len(res1) == 24
    m1, m4 = ex1.memory, ex4.memory
    assert len(m1) == len(m4) and np.array_equal(m1.rows_host()[1], m4.rows_host()[1])
    assert [i.replace(rid1, "") for i in m1.ids] == [i.replace(rid4, "") for i in m4.ids]
    # the reference, chunk by chunk
    model = N.GatedMemory(768, "f16")
    for c, r in enumerate(res1):
        batch = emb_bits[5 * c:5 * c + 5]
        keep, row_of = model.append_novel(batch, tau, known=model.known(batch))
        assert r["embedding_rows"] == row_of.tolist() and r["stored_frames"] == int(keep.sum()), c
        assert set(r) >= {"time", "content", "chunk_idx", "embedding_rows", "similar", "stored_frames"}
    stored = m1.rows_host()[1]
    assert len(m1) == sum(r["stored_frames"] for r in res1) == model.total == len(m1.ids)
    assert np.array_equal(stored, model.rows)
    first = np.r_[True, owner[1:] != owner[:-1]]
    assert 0.05 * 120 <= model.total <= 0.95 * 120 and model.total == int(first.sum())
    # every embedding_rows entry is a valid row: the frame's own, or one that scores above tau against it
    kept_ids = []
    for c, r in enumerate(res1):
        for i, row in enumerate(r["embedding_rows"]):
            f = 5 * c + i
            assert 0 <= row < len(m1)
            if np.array_equal(stored[row], emb_bits[f]) and first[f]:
                kept_ids.append(f"{rid1}_{c}_{i}")
                assert m1.id_of(row) == kept_ids[-1] and m1.meta_of(row)["batch_id"] == c
            else:
                assert cref.cosine_matrix(emb_bits[f:f + 1], stored[row:row + 1])[0, 0] > tau
    assert m1.ids == kept_ids                                 # ids for the kept rows only, in row order
    # `similar` is computed before the gate: a dropped frame's first neighbour is the row it duplicates
    for c, r in enumerate(res1[1:], 1):
        for i, row in enumerate(r["embedding_rows"]):
            if row < sum(x["stored_frames"] for x in res1[:c]):          # suppressed by a row stored before this chunk
                assert r["similar"][i][0][0] == m1.id_of(row).replace(rid1, "RUN")
    # the ungated extractor stores every frame and writes no stored_frames
    res_off, _ = _process(ex_off, clip, tmp_path / "off.json")
    assert len(ex_off.memory) == 120 and "stored_frames" not in res_off[0]
    assert res_off[3]["embedding_rows"] == list(range(15, 20))
    # snapshot -> restore: a gated memory is an ordinary memory
    snap = str(tmp_path / "gated.npz")
    m1.snapshot(snap)
    back = EmbeddingMemory.restore(snap, capacity=512)
    assert len(back) == len(m1) and back.ids == m1.ids
    q = all_emb[[0, 17, 63, 119]]
    for a, b in zip(m1.topk(q, 6), back.topk(q, 6)):
        assert torch.equal(a, b)
    nov_a, nov_b = m1.append_novel(all_emb[:40], tau), back.append_novel(all_emb[:40], tau)
    assert nov_a.kept == nov_b.kept == 0 and torch.equal(nov_a.row_of, nov_b.row_of)
