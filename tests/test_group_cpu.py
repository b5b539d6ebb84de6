"""CPU: the grouped top-k oracle (tests/group_ref.py) against its plain-loop restatement, and the host-side rules of
the grouped search (config default, argument errors, the sharded refusal, the snapshot key field)."""
import numpy as np
import pytest

from tests import group_ref as G


def _scores(rng, Q, n, ties=True):
    s = np.round(rng.uniform(-1, 1, (Q, n)), 2 if ties else 12)  # 2 decimals: many exact ties
    return s


@pytest.mark.parametrize("score_mode", [0, 1])
@pytest.mark.parametrize("min_score", [None, 0.2, 0.7])
@pytest.mark.parametrize("seed", range(6))
def test_vectorised_oracle_equals_plain_loops(seed, min_score, score_mode):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 80))
    sizes = []
    while sum(sizes) < n:
        sizes.append(int(rng.integers(1, 9)))            # ragged groups
    keys = np.concatenate([[rng.integers(0, 3)] * s for s in sizes])[:n]  # small key range: keys reappear
    scores = _scores(rng, 4, n)
    for k in (1, 3, 10, 64):
        a = G.grouped_topk_from_scores(scores, keys, k, score_mode, min_score, base=5)
        b = G.grouped_topk_py(scores, keys, k, score_mode, min_score, base=5)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_group_ids_runs_and_reappearing_keys():
    assert G.group_ids([4, 4, 9, 4, 4, -1]).tolist() == [0, 0, 1, 2, 2, 3]
    assert G.group_ids([]).tolist() == []


def test_ties_lower_representative_and_cross_group_order():
    scores = np.array([[0.5, 0.9, 0.9, 0.9, 0.1, 0.9]])
    keys = [0, 0, 0, 1, 1, 2]
    r, s, k = G.grouped_topk_from_scores(scores, keys, 4)
    assert r.tolist() == [[1, 3, 5, -1]] and k.tolist() == [[0, 1, 2, -1]] and s[0, 3] == 0.0


def test_zero_rows_and_zero_query_score_zero():
    q = np.zeros((1, 128), np.float16)
    rows = np.random.default_rng(0).standard_normal((10, 128)).astype(np.float16)
    rows[4] = 0
    r, s, _ = G.grouped_topk(q.view(np.uint16), rows.view(np.uint16), [0] * 3 + [1] * 3 + [2] * 4, 3)
    assert r.tolist() == [[0, 3, 6]] and (s == 0.0).all()   # every score 0.0: the first row of each group


def test_singleton_groups_equal_the_row_ranking():
    from oracle import cref
    rng = np.random.default_rng(3)
    q = rng.standard_normal((3, 128)).astype(np.float16)
    rows = rng.standard_normal((200, 128)).astype(np.float16)
    rows[50] = rows[10]
    r0, s0 = cref.cosine_topk(q.view(np.uint16), rows.view(np.uint16), 20)
    r1, s1, _ = G.grouped_topk(q.view(np.uint16), rows.view(np.uint16), np.arange(200), 20)
    assert np.array_equal(r0, r1) and np.array_equal(s0.view(np.int64), s1.view(np.int64))


def test_ring_window_cut_through_a_group():
    """A window [base, base+n) of a longer history: the cut group is made of its surviving rows; ids keep counting."""
    rng = np.random.default_rng(5)
    scores = _scores(rng, 2, 40)
    keys = np.repeat(np.arange(8), 5)
    full = G.grouped_topk_py(scores[:, 13:], keys[13:], 6, base=13)
    cut = G.grouped_topk_from_scores(scores[:, 13:], keys[13:], 6, base=13)
    for x, y in zip(full, cut):
        assert np.array_equal(x, y)
    assert 13 <= cut[0][cut[0] >= 0].min()


def test_config_default_is_off():
    from vidmem import config as cfg
    assert cfg.MEMORY_DEFAULTS["group_by"] is None
    assert cfg.from_dict({}).memory.group_by is None


def test_build_memory_rejects_unknown_group_by():
    from vidmem import config as cfg
    from vidmem.extractor import build_memory

    class Enc:
        dtype_name, out_dim = "f16", 768
    with pytest.raises(ValueError, match="group_by"):
        build_memory(cfg.from_dict({"memory": {"group_by": "scene"}}).memory, Enc())


class _FakeMemory:
    grouped = False
    dim = 768
    searchable = 10


def test_distinct_needs_a_grouped_memory():
    from vidmem import _lib
    from vidmem.similarity import HipPreLLMSimilarity, HipVectorSearch, batch_similarities
    with pytest.raises(ValueError, match="grouped"):
        HipVectorSearch(_FakeMemory(), object(), object(), score_mode=_lib.VM_SCORE_RAW, distinct=True)
    with pytest.raises(ValueError, match="grouped"):
        HipPreLLMSimilarity(_FakeMemory(), object(), distinct=True)
    with pytest.raises(ValueError, match="grouped"):
        batch_similarities(_FakeMemory(), [[0.0] * 768], 3, distinct=True)


def test_group_keys_need_a_grouped_memory():
    from vidmem.memory import EmbeddingMemory
    mem = EmbeddingMemory.__new__(EmbeddingMemory)   # host rules only: no device handle
    mem.grouped = False
    with pytest.raises(ValueError, match="grouped"):
        mem._group_keys_for(3, 7)
    with pytest.raises(ValueError, match="grouped"):
        mem.topk_grouped([[0.0] * 8], 3)


def test_sharded_retriever_refuses_grouped_search():
    import torch
    from vidmem.dist import ShardedRetriever
    r = ShardedRetriever(_FakeMemory(), rank=0, world=2, local_topk=lambda *a: None, merge=lambda *a: None)
    with pytest.raises(ValueError, match="span shards"):
        r.search_grouped(torch.zeros(1, 768), 3)


def test_unit_interval_ranks_raw_scores_then_maps():
    """Two raw scores one ulp apart map to one (1 + s) / 2 value: the raw order decides (as the kernels rank)."""
    a = 0.75
    b = np.nextafter(a, 1.0)
    assert (1.0 + a) / 2.0 == (1.0 + b) / 2.0
    scores = np.array([[a, 0.1, b, 0.2]])
    keys = [0, 0, 1, 1]
    for fn in (G.grouped_topk_from_scores, G.grouped_topk_py):
        r, s, k = fn(scores, keys, 2, score_mode=1)
        assert r.tolist() == [[2, 0]] and k.tolist() == [[1, 0]] and s[0, 0] == s[0, 1]
