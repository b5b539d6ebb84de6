"""GPU, end to end: ``consolidate`` keeps a small summary memory beside a tagged, grouped frame memory - one centroid row
per scene - and the existing searches run on it unchanged (memory.py)."""
import numpy as np
import pytest
import torch

from tests import summary_ref as S

pytestmark = pytest.mark.gpu


def test_consolidate_into_a_summary_memory_and_search_it():
    from tests.support import clustered, group_sizes
    from vidmem.memory import EmbeddingMemory, make_tag, scope_of
    D, dtype = 768, "f16"
    sizes = group_sizes(40, "ragged", 8)
    rows, gid = clustered(sizes, D, dtype, seed=41, device="cpu")
    n = rows.shape[0]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    gid = gid.numpy().astype(np.int64)
    source = (gid >= 20).astype(np.int64)                       # two videos of 20 scenes each
    tags = np.array([make_tag(int(s), 40 * i) for i, s in enumerate(source)], np.int64)
    frames = EmbeddingMemory(n + 64, D, dtype, grouped=True, tagged=True)
    first = 30                                                   # scenes 0 .. 29 now, the rest later
    upto = int(starts[first])
    frames.append(rows[:upto], ids=[f"frame_{i}" for i in range(upto)], group=torch.from_numpy(gid[:upto] + 500),
                  tag=torch.from_numpy(tags[:upto]))
    summ = EmbeddingMemory(256, D, dtype, grouped=True, tagged=True)
    s1, at1 = frames.consolidate(summ)
    assert at1 == 0 and s1.count == first and len(summ) == first
    bits = rows.contiguous().view(torch.int16).numpy().view(np.uint16)
    want = S.summarize(bits[:upto], gid[:upto] + 500, dtype)
    assert np.array_equal(s1.centroids.view(torch.int16).cpu().numpy().view(np.uint16), want.centroids)
    assert np.array_equal(s1.key_rows.cpu().numpy(), want.key_rows)
    # what the summary memory holds: the centroid bits, the source group's key, the key row's tag, id and meta
    assert np.array_equal(summ.rows_host()[1], want.centroids)
    assert np.array_equal(summ.group_keys_host(), want.keys) and np.array_equal(summ.tags_host(), tags[want.key_rows])
    for g in (0, 7, first - 1):
        k = int(want.key_rows[g])
        assert summ.id_of(g) == f"frame_{k}"
        m = summ.meta_of(g)
        assert (m["first_row"], m["last_row"], m["key_row"]) == (int(starts[g]), int(starts[g + 1]) - 1, k)
        assert m["key_score"] == float(want.key_scores[g]) and starts[g] <= k < starts[g + 1]
    # a planted scene's query finds that scene's summary first
    scenes = [3, 12, 25]
    q = torch.stack([rows[int(starts[g]) + sizes[g] // 2] for g in scenes])
    scores, hit = summ.topk(q, 3)
    assert hit[:, 0].tolist() == scenes and (scores[:, 0] > 0.9).all() and (scores[:, 1] < 0.5).all()
    # the inherited tags: a search of video 1 sees only its scenes
    sc_scores, sc_hit = summ.topk_scoped(q, 3, scope_of(1))
    assert (sc_hit >= 20).all() and sc_hit[2, 0].item() == 25 and set(sc_hit[0].tolist()).isdisjoint({3})
    sc_scores0, sc_hit0 = summ.topk_scoped(q, 3, scope_of(0))
    assert (sc_hit0 < 20).all() and sc_hit0[:2, 0].tolist() == [3, 12]
    # more frames arrive; a second consolidate from first_group = count adds only the new groups
    frames.append(rows[upto:], ids=[f"frame_{i}" for i in range(upto, n)], group=torch.from_numpy(gid[upto:] + 500),
                  tag=torch.from_numpy(tags[upto:]))
    s2, at2 = frames.consolidate(summ, first_group=s1.count)
    assert at2 == first and s2.count == 40 and s2.first_rows.numel() == 10 and len(summ) == 40
    whole = S.summarize(bits, gid + 500, dtype)
    assert np.array_equal(summ.rows_host()[1], whole.centroids) and np.array_equal(summ.group_keys_host(), whole.keys)
    assert summ.meta_of(39)["last_row"] == n - 1 and summ.id_of(35) == f"frame_{int(whole.key_rows[35])}"
    q2 = rows[int(starts[33]) + 1].unsqueeze(0)
    assert summ.topk(q2, 1)[1].item() == 33
    s3, at3 = frames.consolidate(summ, first_group=s2.count)          # nothing new: nothing appended
    assert s3.first_rows.numel() == 0 and at3 == 40 and len(summ) == 40
