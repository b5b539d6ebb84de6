"""CPU: the two statements of the scoped top-k oracle (tests/scope_ref.py) against each other, the tag helpers, and the
host-side rules of the scoped search (config default, argument errors, exported symbols, no device -> no memory)."""
import ctypes as C

import numpy as np
import pytest

from tests import scope_ref as S


def _case(seed, n=3000, D=768, Q=12):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, D)).astype(np.float16)
    for i in range(0, 200, 7):                       # planted exact duplicates, in and out of any scope
        rows[rng.integers(0, n)] = rows[i]
    q = rows[rng.integers(0, n, Q)].astype(np.float32) + 0.1 * rng.standard_normal((Q, D)).astype(np.float32)
    q = q.astype(np.float16)
    q[3] = rows[0]
    q[4] = 0
    tags = rng.integers(0, 40, n).astype(np.int64)   # non-monotone
    tags[rng.integers(0, n, 50)] = S.INT64_MIN
    scopes = [(int(a), int(a + w)) for a, w in zip(rng.integers(0, 40, Q), rng.integers(0, 12, Q))]
    scopes[0] = (50, 60)                             # no row
    scopes[1] = (9, 3)                               # lo > hi
    scopes[2] = (S.INT64_MIN, S.INT64_MAX)
    return q.view(np.uint16), rows.view(np.uint16), tags, scopes


@pytest.mark.parametrize("score_mode,min_score", [(0, None), (0, 0.3), (1, 0.65)])
@pytest.mark.parametrize("seed", [0, 1])
def test_two_statements_agree(seed, score_mode, min_score):
    q, rows, tags, scopes = _case(seed)
    for k in (1, 10, 64):
        ra, sa = S.scoped_topk(q, rows, tags, scopes, k, "f16", score_mode, min_score, base=7)
        rb, sb = S.scoped_topk_matrix(q, rows, tags, scopes, k, "f16", score_mode, min_score, base=7)
        assert np.array_equal(ra, rb)
        assert np.array_equal(sa.view(np.int64), sb.view(np.int64))
        assert (ra[0] == -1).all() and (ra[1] == -1).all() and (sa[:2] == 0.0).all()
        assert (ra[2:] >= 7).any()
    r, _ = S.scoped_topk(q, rows, tags, scopes, 64, "f16", score_mode, min_score)
    lo, hi = S.scope_arrays(scopes, q.shape[0])
    for qi in range(q.shape[0]):                     # only in-scope rows are ever returned
        got = r[qi][r[qi] >= 0]
        assert S.scope_mask(tags[got], lo[qi], hi[qi]).all()


def test_whole_scope_equals_the_row_ranking():
    from oracle import cref
    q, rows, tags, _ = _case(5, n=500, D=128, Q=6)
    r0, s0 = cref.cosine_topk(q, rows, 20)
    r1, s1 = S.scoped_topk(q, rows, tags, (S.INT64_MIN, S.INT64_MAX), 20)
    assert np.array_equal(r0, r1) and np.array_equal(s0.view(np.int64), s1.view(np.int64))


def test_ties_in_scope_by_row_id_and_zero_query():
    scores = np.array([[0.9, 0.9, 0.5, 0.9, 0.9], [0.0] * 5])
    tags = [1, 2, 2, 2, 1]
    r, s = S.scoped_topk_from_scores(scores, tags, (2, 2), 3)
    assert r.tolist() == [[1, 3, 2], [1, 2, 3]] and s[1].tolist() == [0.0] * 3


def test_make_tag_and_scope_of():
    from vidmem.memory import INT64_MAX, INT64_MIN, SCOPE_ALL, make_tag, scope_of
    assert make_tag(0, 0) == 0 and make_tag(3, 5) == (3 << 40) | 5
    assert scope_of(3) == (3 << 40, (3 << 40) | ((1 << 40) - 1))
    assert scope_of(3, 180_000, 300_000) == ((3 << 40) | 180_000, (3 << 40) | 300_000)
    assert scope_of(3, 180_000) == ((3 << 40) | 180_000, (3 << 40) | ((1 << 40) - 1))
    assert scope_of(2)[1] + 1 == scope_of(3)[0]                   # sources tile the tag line without gaps
    top = make_tag((1 << 22) - 1, (1 << 40) - 1)
    assert top == (1 << 62) - 1 and top < INT64_MAX
    assert (top >> 40, top & ((1 << 40) - 1)) == ((1 << 22) - 1, (1 << 40) - 1)   # round trip
    lo, hi = scope_of(7, 10, 20)
    assert lo <= make_tag(7, 10) <= hi and lo <= make_tag(7, 20) <= hi
    assert not lo <= make_tag(7, 21) <= hi and not lo <= make_tag(6, 15) <= hi
    assert SCOPE_ALL == (INT64_MIN, INT64_MAX)
    for bad in [(-1, 0), (1 << 22, 0), (0, -1), (0, 1 << 40)]:
        with pytest.raises(ValueError):
            make_tag(*bad)
    with pytest.raises(ValueError):
        scope_of(0, -5)
    with pytest.raises(ValueError):
        scope_of(1 << 22)


def test_config_default_is_off():
    from vidmem import config as cfg
    assert cfg.MEMORY_DEFAULTS["tag_by"] is None
    assert cfg.from_dict({}).memory.tag_by is None
    assert cfg.from_dict({"memory": {"tag_by": "time"}}).memory.tag_by == "time"


def test_build_memory_rejects_unknown_tag_by():
    from vidmem import config as cfg
    from vidmem.extractor import build_memory

    class Enc:
        dtype_name, out_dim = "f16", 768
    with pytest.raises(ValueError, match="tag_by"):
        build_memory(cfg.from_dict({"memory": {"tag_by": "scene"}}).memory, Enc())


class _FakeMemory:
    grouped = False
    tagged = False
    dim = 768
    searchable = 10


class _FakeTaggedGrouped(_FakeMemory):
    grouped = True
    tagged = True


def test_scope_needs_a_tagged_memory_and_excludes_distinct():
    from vidmem import _lib
    from vidmem.fusion import HipHybridMixin
    from vidmem.similarity import HipPreLLMSimilarity, HipVectorSearch, batch_similarities
    sc = (0, 10)
    with pytest.raises(ValueError, match="tagged"):
        HipVectorSearch(_FakeMemory(), object(), object(), score_mode=_lib.VM_SCORE_RAW, scope=sc)
    with pytest.raises(ValueError, match="tagged"):
        HipPreLLMSimilarity(_FakeMemory(), object(), scope=sc)
    with pytest.raises(ValueError, match="tagged"):
        batch_similarities(_FakeMemory(), [[0.0] * 768], 3, scope=sc)
    with pytest.raises(ValueError, match="distinct"):
        HipVectorSearch(_FakeTaggedGrouped(), object(), object(), score_mode=_lib.VM_SCORE_RAW, distinct=True, scope=sc)
    with pytest.raises(ValueError, match="distinct"):
        HipPreLLMSimilarity(_FakeTaggedGrouped(), object(), distinct=True, scope=sc)
    with pytest.raises(ValueError, match="distinct"):
        batch_similarities(_FakeTaggedGrouped(), [[0.0] * 768], 3, distinct=True, scope=sc)

    class R(HipHybridMixin):
        config, embedder = object(), object()
    with pytest.raises(ValueError, match="tagged"):
        R().attach_memory(_FakeMemory(), score_mode=_lib.VM_SCORE_RAW, scope=sc)
    assert HipVectorSearch(_FakeTaggedGrouped(), object(), object(), score_mode=_lib.VM_SCORE_RAW, scope=sc).scope == sc


def test_tags_and_scoped_search_need_a_tagged_memory():
    from vidmem.memory import EmbeddingMemory
    mem = EmbeddingMemory.__new__(EmbeddingMemory)   # host rules only: no device handle
    mem.tagged = False
    with pytest.raises(ValueError, match="tagged"):
        mem._tags_for(3, 7)
    with pytest.raises(ValueError, match="tagged"):
        mem.topk_scoped([[0.0] * 8], 3, (0, 1))
    with pytest.raises(ValueError, match="tagged"):
        mem.tags_host()
    mem.tagged = True
    for k in (0, 65):
        with pytest.raises(ValueError, match="k"):
            mem.topk_scoped([[0.0] * 8], k, (0, 1))
    assert mem._tags_for(3, None) is None


def test_library_exports_the_scoped_symbols_and_abi_4():
    from vidmem import _lib
    L = _lib.lib()
    assert L.vm_abi_version() == 4
    for sym in ("vm_memory_create_tagged", "vm_memory_append_tagged", "vm_memory_tags",
                "vm_topk_scoped_workspace_bytes", "vm_topk_cosine_scoped", "vm_topk_cosine_scoped_exact"):
        assert sym in _lib.SYMBOLS
        getattr(L, sym)
    assert L.vm_memory_tags(None) is None and L.vm_topk_scoped_workspace_bytes(None, 1, 1) == 0
    assert L.vm_topk_cosine_scoped(None, None, 1, 1, None, None, 0, 0.0, 0, 1, 0, None, None, None, None, None, 0,
                                   None) == _lib.VM_ERR_INVALID


def test_tagged_constructor_without_a_gpu_fails_with_no_device():
    import torch
    from vidmem import _lib
    from vidmem.memory import EmbeddingMemory
    if torch.cuda.is_available():
        mem = EmbeddingMemory(16, 128, "f16", tagged=True)      # with a device the same call succeeds
        assert mem.tagged and C.c_void_p(mem.L.vm_memory_tags(mem.handle)).value
        return
    with pytest.raises(_lib.VidmemError) as e:
        EmbeddingMemory(16, 128, "f16", tagged=True)
    assert e.value.code == _lib.VM_ERR_NO_DEVICE
