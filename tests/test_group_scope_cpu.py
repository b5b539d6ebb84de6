"""CPU: the scoped grouped top-k's reference (tests/group_scope_ref.py) against itself and against its two parents'
references, and the host rules of the adapters.  No GPU call is made here."""
import asyncio

import numpy as np
import pytest

from tests import group_ref as G
from tests import group_scope_ref as GS
from tests import scope_ref as S

ALL = (S.INT64_MIN, S.INT64_MAX)


def _same(a, b):
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        if x.dtype == np.float64:
            assert np.array_equal(x.view(np.int64), y.view(np.int64))
        else:
            assert np.array_equal(x, y)


def _random_case(seed, n=400, Q=7):
    rng = np.random.default_rng(seed)
    scores = np.round(rng.uniform(-1, 1, (Q, n)), 2)              # two decimals: plenty of exact ties
    keys = np.repeat(np.arange(n), rng.integers(1, 9, n))[:n].astype(np.int64)
    keys[keys % 11 == 3] = 3                                      # a key that comes back opens a new group
    tags = rng.integers(0, 40, n).astype(np.int64)
    scopes = [(int(a), int(a + w)) for a, w in zip(rng.integers(-5, 40, Q), rng.integers(-2, 25, Q))]
    return scores, keys, tags, scopes


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("score_mode,min_score", [(0, None), (0, 0.3), (1, 0.65), (1, None)])
def test_two_statements_agree_on_random_inputs(seed, score_mode, min_score):
    scores, keys, tags, scopes = _random_case(seed)
    for k in (1, 5, 64):
        _same(GS.group_scoped_topk_from_scores(scores, keys, tags, scopes, k, score_mode, min_score, base=17),
              GS.group_scoped_topk_py(scores, keys, tags, scopes, k, score_mode, min_score, base=17))


def test_adversarial_inputs():
    #        group 0        | group 1     | group 2 | group 3
    keys = np.array([5, 5, 5, 6, 6, 6, 6, 7, 7, 5], np.int64)
    tags = np.array([0, 9, 0, 9, 0, 9, 0, 9, 9, 0], np.int64)
    scores = np.array([[.5, .9, .5, .8, .2, .7, .2, .95, .6, .5],            # each group's best row has tag 9
                       [-.5, -.1, -.5, -.8, -.2, -.7, -.2, -.9, -.6, -.5]])  # every score negative
    for sc, k in (((0, 0), 4), ((9, 9), 4), (ALL, 4), ((1, 8), 2), ((3, 1), 2)):
        _same(GS.group_scoped_topk_from_scores(scores, keys, tags, sc, k), GS.group_scoped_topk_py(scores, keys, tags, sc, k))
    r, s, kk = GS.group_scoped_topk_from_scores(scores, keys, tags, (0, 0), 4)
    # tag 0 only: group 0 scores .5 at its lowest tied row 0 (row 1, its best, is hidden); group 2 has no in-scope row
    # and is absent; group 3 (key 5 again) ties group 0 and loses on the row id; padding is -1 / 0.0 / -1
    assert r[0].tolist() == [0, 9, 4, -1] and s[0].tolist() == [.5, .5, .2, 0.0] and kk[0].tolist() == [5, 5, 6, -1]
    # all negative: negative scores are returned, an absent group never shows up at 0.0
    assert r[1].tolist() == [4, 0, 9, -1] and s[1].tolist() == [-.2, -.5, -.5, 0.0]
    # a hidden row between two in-scope rows of group 1 does not split it: one hit for rows 4 and 6
    r, _, _ = GS.group_scoped_topk_from_scores(scores[:1], keys, tags, (0, 0), 4)
    assert sorted(r[0].tolist()).count(4) == 1 and 6 not in r[0].tolist()
    # hiding group 2 does not merge its neighbours... nor do groups 0 and 3, which share key 5
    r, _, _ = GS.group_scoped_topk_from_scores(scores[:1], np.array([5, 6, 5], np.int64), np.array([0, 9, 0], np.int64),
                                               (0, 0), 3)
    assert r[0].tolist() == [0, 2, -1]
    # an empty scope
    r, s, kk = GS.group_scoped_topk_from_scores(scores, keys, tags, (3, 1), 2)
    assert (r == -1).all() and (s == 0.0).all() and (kk == -1).all()


@pytest.mark.parametrize("seed", range(4))
def test_whole_scope_equals_the_grouped_reference(seed):
    scores, keys, tags, _ = _random_case(seed)
    for score_mode, min_score in ((0, None), (1, 0.6)):
        _same(GS.group_scoped_topk_from_scores(scores, keys, tags, ALL, 10, score_mode, min_score, base=3),
              G.grouped_topk_from_scores(scores, keys, 10, score_mode, min_score, base=3))


@pytest.mark.parametrize("seed", range(4))
def test_singleton_groups_equal_the_scoped_reference(seed):
    scores, _, tags, scopes = _random_case(seed)
    keys = np.arange(scores.shape[1], dtype=np.int64)
    for score_mode, min_score in ((0, None), (1, 0.6)):
        r, s, _ = GS.group_scoped_topk_from_scores(scores, keys, tags, scopes, 10, score_mode, min_score, base=3)
        _same((r, s), S.scoped_topk_from_scores(scores, tags, scopes, 10, score_mode, min_score, base=3))


# ---- adapters -------------------------------------------------------------------------------------------------------
class _Refusing:
    """Grouped and tagged, but without topk_grouped_scoped (the stand-ins of tests/test_scope_cpu.py)."""
    grouped = True
    tagged = True
    dim = 4
    searchable = 6


class _Routing(_Refusing):
    def __init__(self):
        self.calls = []

    def __len__(self):
        return 6

    def id_of(self, r):
        return f"row{r}"

    def meta_of(self, r):
        return {"time": r, "content": f"c{r}"}

    def tags_host(self):
        return np.array([1, 0, 1, 1, 0, 1], np.int64)

    def group_keys_host(self):
        return np.array([7, 7, 7, 8, 9, 7], np.int64)

    def topk_grouped_scoped(self, q, k, scope, min_score=None, score_mode=0, exact=False):
        import torch
        self.calls.append((len(q), k, scope, min_score, score_mode))
        Q = len(q)
        return (torch.full((Q, k), 0.5, dtype=torch.float64), torch.arange(k).repeat(Q, 1),
                torch.zeros((Q, k), dtype=torch.int64))

    def topk_scoped(self, *a, **kw):
        raise AssertionError("distinct=True with a scope must not take the row search")

    topk_grouped = topk = topk_scoped


class _Cfg:
    top_k_chunk_with_batch_similarity = 2
    top_k_chunks = 3


class _Embedder:
    async def aembed_query(self, query):
        return [1.0, 0.0, 0.0, 0.0]


def test_adapters_route_distinct_with_scope_to_the_new_search():
    from vidmem import _lib
    from vidmem.fusion import HipHybridMixin
    from vidmem.similarity import HipPreLLMSimilarity, HipVectorSearch, batch_similarities
    sc = (1, 1)
    mem = _Routing()
    out = batch_similarities(mem, [[1.0, 0.0, 0.0, 0.0], [1.0, 2.0]], 2, distinct=True, scope=sc)
    assert mem.calls == [(1, 2, sc, None, 0)]
    assert out[0] == [("row0", 0.5), ("row1", 0.5)]
    # the wrong-length query: the first in-scope row of each of the first 2 in-scope groups (rows 0 and 2 share group 0)
    assert out[1] == [("row0", 0.0), ("row3", 0.0)]
    assert batch_similarities(mem, [[1.0, 2.0]], 5, distinct=True, scope=sc)[0] == \
        [("row0", 0.0), ("row3", 0.0), ("row5", 0.0)]

    mem = _Routing()
    sim = HipPreLLMSimilarity(mem, _Cfg(), distinct=True, scope=sc)
    asyncio.run(sim._calculate_batch_similarities([[0.0, 1.0, 0.0, 0.0]]))
    assert mem.calls == [(1, 2, sc, None, 0)]

    mem = _Routing()
    vs = HipVectorSearch(mem, _Embedder(), _Cfg(), score_mode=_lib.VM_SCORE_UNIT_INTERVAL, min_score=0.4, distinct=True,
                         scope=sc)
    chunks = asyncio.run(vs._vector_search_chunks(None, "a question"))
    assert mem.calls == [(1, 3, sc, 0.4, _lib.VM_SCORE_UNIT_INTERVAL)]
    assert [c["id"] for c in chunks] == ["row0", "row1", "row2"]

    class R(HipHybridMixin):
        config, embedder = _Cfg(), _Embedder()
    mem = _Routing()
    r = R().attach_memory(mem, score_mode=_lib.VM_SCORE_RAW, distinct=True, scope=sc)
    asyncio.run(r._hip._vector_search_chunks(None, "a question"))
    assert mem.calls == [(1, 3, sc, 0.3, _lib.VM_SCORE_RAW)]


def test_adapters_refuse_distinct_with_scope_without_the_new_search():
    from vidmem import _lib
    from vidmem.similarity import HipPreLLMSimilarity, HipVectorSearch, batch_similarities
    sc = (0, 10)
    for make in (lambda: HipVectorSearch(_Refusing(), object(), object(), score_mode=_lib.VM_SCORE_RAW, distinct=True,
                                         scope=sc),
                 lambda: HipPreLLMSimilarity(_Refusing(), object(), distinct=True, scope=sc),
                 lambda: batch_similarities(_Refusing(), [[0.0] * 4], 3, distinct=True, scope=sc)):
        with pytest.raises(ValueError, match="distinct.*topk_grouped_scoped"):
            make()


def test_memory_refuses_a_memory_that_is_not_both_grouped_and_tagged():
    from vidmem.memory import EmbeddingMemory
    mem = EmbeddingMemory.__new__(EmbeddingMemory)   # host rules only: no device handle
    for grouped, tagged in ((False, False), (True, False), (False, True)):
        mem.grouped, mem.tagged = grouped, tagged
        with pytest.raises(ValueError, match="grouped and tagged"):
            mem.topk_grouped_scoped([[0.0] * 8], 3, (0, 1))
    mem.grouped = mem.tagged = True
    for k in (0, 65):
        with pytest.raises(ValueError, match="k"):
            mem.topk_grouped_scoped([[0.0] * 8], k, (0, 1))


def test_library_exports_the_new_symbols():
    from vidmem import _lib
    L = _lib.lib()
    for name in ("vm_topk_grouped_scoped_workspace_bytes", "vm_topk_cosine_grouped_scoped",
                 "vm_topk_cosine_grouped_scoped_exact"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert L.vm_abi_version() == 4
