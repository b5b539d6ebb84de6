"""GPU, end to end: two synthetic videos in which one scene recurs (tests/diverse_ref.py ``e2e_videos``).

``similarity.batch_similarities`` spends its k context slots on frames of the recurring scene;
``similarity.diverse_similarities`` at lam = 0.5 returns the ``(id, score)`` lists of statement (A) of the oracle, and
those cover more distinct scenes - by a count taken from the oracle before any search."""
import numpy as np
import pytest
import torch

from oracle import cref
from tests import diverse_ref as DR

pytestmark = pytest.mark.gpu


def test_diverse_hits_cover_more_scenes_and_equal_the_oracle():
    from vidmem import similarity
    from vidmem.memory import EmbeddingMemory
    bits, scene, video = DR.e2e_videos()
    qbits = DR.e2e_queries()
    n, D, k = bits.shape[0], DR.E2E_D, DR.E2E_K
    names = [f"{'AB'[v]}{i}" for i, v in enumerate(video)]
    scene_of = dict(zip(names, scene.tolist()))
    # the oracle first: what plain top-k covers, what the diverse search must return and cover
    plain_r, _ = cref.cosine_topk(qbits, bits, k)
    pool = min(64, 4 * k)                                           # the default
    want_r, want_s, _ = DR.diverse_topk(qbits, bits, None, k, pool, 0.5, sim=DR.sim_matrix(bits))
    plain_scenes = [len(set(scene[r].tolist())) for r in plain_r]
    want_scenes = [len(set(scene[r].tolist())) for r in want_r]
    assert plain_scenes == [1] * 3 and all(w >= 3 for w in want_scenes)

    rows = torch.from_numpy(bits.view(np.int16).copy()).view(torch.float16).cuda()
    queries = torch.from_numpy(qbits.view(np.int16).copy()).view(torch.float16).cuda()
    mem = EmbeddingMemory(64, D, "f16")
    half = int((video == 0).sum())
    mem.append(rows[:half], ids=names[:half])
    mem.append(rows[half:], ids=names[half:])
    plain = similarity.batch_similarities(mem, list(queries), k)
    got = similarity.diverse_similarities(mem, queries, k, lam=0.5)
    assert [[i for i, _ in hits] for hits in got] == [[names[r] for r in row] for row in want_r.tolist()]
    assert [[v for _, v in hits] for hits in got] == want_s.tolist()
    for c in range(3):
        assert len({scene_of[i] for i, _ in plain[c]}) == plain_scenes[c]
        assert len({scene_of[i] for i, _ in got[c]}) == want_scenes[c] > plain_scenes[c]
        assert got[c][0] == plain[c][0]                             # the best frame leads either list
    # lam = 1 is the plain answer; a mask and a threshold pass through; an empty memory yields empty lists
    assert similarity.diverse_similarities(mem, queries, k, lam=1.0) == plain
    only_b = mem.mask_where(lambda r, i, m: i.startswith("B"))
    sel = np.broadcast_to(video == 1, (3, n))
    want_r, want_s, _ = DR.diverse_topk(qbits, bits, sel, k, 12, 0.5, min_score=0.5, sim=DR.sim_matrix(bits))
    got = similarity.diverse_similarities(mem, queries, k, pool=12, lam=0.5, mask=only_b, min_score=0.5)
    assert [[i for i, _ in hits] for hits in got] == [[names[r] for r in row if r >= 0] for row in want_r.tolist()]
    assert [[v for _, v in hits] for hits in got] == [[v for v, r in zip(vs, rs) if r >= 0]
                                                      for vs, rs in zip(want_s.tolist(), want_r.tolist())]
    assert all(i.startswith("B") for hits in got for i, _ in hits)
    assert similarity.diverse_similarities(EmbeddingMemory(16, D, "f16"), queries, k) == [[], [], []]
    mem.close()
