"""CPU: the one owner rule of the memory's scratch buffers (vidmem/scratch.py, ``EmbeddingMemory._resolve``) on every
kind, against a stand-in library whose sizing calls grow with their arguments, and the argument coercions that every
memory operation shares."""
import pytest
import torch

from tests.host_memory import SizingLibrary, host_memory, scratch_buffers


def _memory(capacity=16):
    return host_memory(grouped=True, tagged=True, capacity=capacity, library=SizingLibrary())


def _kinds():
    from vidmem import memory as M
    # kind, prepare_* of the memory, a shape, a larger shape
    return {
        "topk": (M.TopkScratch, "prepare_topk", (4, 10), (64, 32)),
        "grouped": (M.GroupedTopkScratch, "prepare_topk_grouped", (4, 10), (64, 32)),
        "scoped": (M.ScopedTopkScratch, "prepare_topk_scoped", (4, 10), (64, 32)),
        "grouped_scoped": (M.GroupedScopedTopkScratch, "prepare_topk_grouped_scoped", (4, 10), (64, 32)),
        "clip": (M.ClipScratch, "prepare_topk_clip", (2, 4, 5), (8, 4, 16)),
        "novelty": (M.NoveltyScratch, "prepare_append_novel", (16,), (64,)),
        "range": (M.RangeScratch, "prepare_range", (4, 8), (16, 64)),
        "events": (M.EventsScratch, "prepare_events", (4,), (32,)),
        "summary": (M.SummaryScratch, "prepare_summaries", (4,), (32,)),
        "erase": (M.EraseScratch, "prepare_erase", (0,), (64,)),
    }


KINDS = ["topk", "grouped", "scoped", "grouped_scoped", "clip", "novelty", "range", "events", "summary", "erase"]


@pytest.mark.parametrize("name", KINDS)
def test_own_scratch_is_kept_while_it_fits_and_replaced_to_grow(name):
    kind, prepare, shape, larger = _kinds()[name]
    mem = _memory()
    first = getattr(mem, prepare)(*shape)
    assert isinstance(first, kind) and first.fits(mem, *shape)
    before = scratch_buffers(first)
    assert "ws" in before and before["ws"][1] >= 256
    assert getattr(mem, prepare)(*shape) is first                       # it fits: the same object
    assert mem._resolve(kind, None, *shape) is first
    grown = getattr(mem, prepare)(*larger)
    assert grown is not first and isinstance(grown, kind) and grown.fits(mem, *larger)
    assert scratch_buffers(first) == before                                    # replaced, never resized in place
    assert set(scratch_buffers(grown)) == set(before)
    assert getattr(mem, prepare)(*larger) is grown


@pytest.mark.parametrize("name", KINDS)
def test_caller_owned_scratch_must_fit(name):
    kind, prepare, shape, larger = _kinds()[name]
    mem = _memory()
    own = getattr(mem, prepare)(*shape)
    before = scratch_buffers(own)
    if name == "erase":       # any segment size serves an erase call: too small = made for a smaller memory
        small, call = kind.for_(_memory(capacity=8)), ()
    else:
        small, call = kind.for_(mem, *shape), larger
    theirs = scratch_buffers(small)
    with pytest.raises(ValueError, match="too small"):
        mem._resolve(kind, small, *call)
    assert getattr(mem, prepare)(*shape) is own and scratch_buffers(own) == before and scratch_buffers(small) == theirs
    fitting = kind.for_(mem, *larger)
    assert mem._resolve(kind, fitting, *call) is fitting                # a caller-owned one that fits is used as it is
    assert getattr(mem, prepare)(*shape) is own


def test_buffers_keep_their_names_types_and_fills():
    from vidmem import memory as M
    mem = _memory()
    want = {
        M.TopkScratch: ((4, 10), {"redo_ws": (torch.uint8, None), "flags": (torch.int32, 0), "uncert": (torch.int32, 0)}),
        M.GroupedTopkScratch: ((4, 10), {"flags": (torch.int32, 0)}),
        M.ScopedTopkScratch: ((4, 10), {"flags": (torch.int32, 0)}),
        M.GroupedScopedTopkScratch: ((4, 10), {"flags": (torch.int32, 0)}),
        M.ClipScratch: ((2, 4, 5), {"flags": (torch.int32, 0), "scores": (torch.float64, 0.0), "rows": (torch.int64, -1)}),
        M.NoveltyScratch: ((16,), {"keep": (torch.int32, 0), "row_of": (torch.int64, 0), "count": (torch.int32, 0)}),
        M.RangeScratch: ((4, 8), {"counts": (torch.int64, 0), "rescored": (torch.int64, 0), "rows": (torch.int64, -1),
                                  "scores": (torch.float64, 0.0)}),
        M.EventsScratch: ((4,), {"count": (torch.int64, 0), "first_rows": (torch.int64, -1), "event_of": (torch.int64, 0),
                                 "links": (torch.float64, 0.0)}),
        M.SummaryScratch: ((4,), {"count": (torch.int64, 0), "first_rows": (torch.int64, -1), "n_rows": (torch.int64, -1),
                                  "keys": (torch.int64, -1), "key_rows": (torch.int64, -1),
                                  "key_scores": (torch.float64, 0.0), "centroids": (torch.float16, 0.0)}),
        M.EraseScratch: ((0,), {"new_row_of": (torch.int64, -1), "erased": (torch.int64, 0)}),
    }
    for kind, (shape, buffers) in want.items():
        s = kind.for_(mem, *shape)
        assert s.ws.dtype == torch.uint8 and s.ws.numel() == 1000 + 64 * sum(s._sized_by(*s.shape))
        assert set(scratch_buffers(s)) == set(buffers) | {"ws"}
        for name, (dtype, fill) in buffers.items():
            t = getattr(s, name)
            assert t.dtype == dtype and (fill is None or (t == fill).all()), (kind.__name__, name)
    assert M.SummaryScratch.for_(mem, 4).centroids.shape == (4, 128)
    assert M.EventsScratch.for_(mem, 4).event_of.numel() == mem.capacity == M.EraseScratch.for_(mem).new_row_of.numel()
    assert M.TopkScratch.for_(mem, 0, 0).ws.numel() == 1000                                       # the library's size
    mem.L = type("Tiny", (), {"__getattr__": lambda self, name: (lambda *a: 0)})()
    assert M.TopkScratch.for_(mem, 4, 10).ws.numel() == 256 == M.EraseScratch.for_(mem).ws.numel()   # the floor


def test_topk_fit_returns_a_new_object_and_carries_the_counter():
    from vidmem.memory import TopkScratch
    mem = _memory()
    first = TopkScratch.for_(mem, 4, 10)
    first.uncert.fill_(7)
    before = scratch_buffers(first)
    assert first.fit(mem, 4, 10) is first and first.fit(mem, 2, 5) is first
    grown = first.fit(mem, 64, 32)
    assert grown is not first and grown.fits(mem, 64, 32) and grown.fits(mem, 4, 10)
    assert grown.uncert.item() == 7 and first.uncert.item() == 7 and scratch_buffers(first) == before
    assert grown.flags.numel() >= 64 and grown.ws.numel() >= first.ws.numel()
    # the memory's own scratch grows the same way: uncertified_count survives the growth
    assert mem.uncertified_count == 0
    mem.prepare_topk(4, 10).uncert.fill_(3)
    assert mem.prepare_topk(64, 32).uncert.item() == 3 and mem.uncertified_count == 3
    mem.reset_uncertified()
    assert mem.uncertified_count == 0


class UnevenLibrary:
    """Sizes that do not grow with their arguments, as the library's do not: nothing above k = 58, and a scan workspace
    that is larger at Q = 128 than at Q = 129 (the block count falls when the queries need one more group)."""

    def __getattr__(self, name):
        if name == "vm_topk_workspace_bytes":
            return lambda handle, Q, k: 0 if k > 58 else (2_098_176 if Q <= 128 else 2_090_752) + 64 * k
        if name == "vm_topk_redo_workspace_bytes":
            return lambda handle, Q, k: 0 if k > 58 else 4096 * Q
        raise AssertionError(f"library call {name}")


def test_topk_scratch_grows_to_what_the_call_needs_and_never_shrinks():
    from vidmem.memory import TopkScratch
    lib = UnevenLibrary()
    # (a) the own scratch was prepared at a k the fast path does not serve: the next fast call gets one that fits
    mem = host_memory(library=lib)
    big_k = mem.prepare_topk(8, 60)
    assert big_k.ws.numel() == 256
    own = mem.prepare_topk(8, 10)
    assert own is not big_k and own.fits(mem, 8, 10) and own.ws.numel() >= lib.vm_topk_workspace_bytes(None, 8, 10)
    assert mem.prepare_topk(8, 10) is own and mem._resolve(TopkScratch, None, 8, 10) is own
    # (b) a smaller need at the larger Q: (129, 5) then (128, 10) on the own scratch
    mem = host_memory(library=lib)
    first = mem.prepare_topk(129, 5)
    second = mem.prepare_topk(128, 10)
    assert second is not first and second.fits(mem, 128, 10) and second.fits(mem, 129, 5)
    assert second.ws.numel() == 2_098_176 + 640 and second.redo_ws.numel() == first.redo_ws.numel() == 4096 * 129
    assert second.flags.numel() == 129 and mem.prepare_topk(129, 5) is second
    # fit itself: whatever the order of the shapes, the result fits the shape that asked and every shape served before
    s = TopkScratch.for_(mem, 4, 60)
    for Q, k in ((4, 10), (129, 5), (128, 10), (16, 58), (1, 1)):
        t = s.fit(mem, Q, k)
        assert t.fits(mem, Q, k) and t.ws.numel() >= s.ws.numel() and t.redo_ws.numel() >= s.redo_ws.numel()
        assert t.flags.numel() >= s.flags.numel()
        s = t


def test_prepare_erase_makes_a_new_scratch_for_another_segment_size():
    mem = _memory()
    a = mem.prepare_erase(64)
    assert mem.prepare_erase(64) is a and mem._resolve(type(a), None) is a       # a call takes the prepared one
    b = mem.prepare_erase(32)                                                     # smaller, and still a new one
    assert b is not a and b.ws.numel() < a.ws.numel() and mem._resolve(type(a), None) is b


def test_last_and_counters_before_any_call():
    mem = _memory()
    for name in ("last_flags", "last_group_flags", "last_scope_flags", "last_group_scope_flags", "last_clip_flags",
                 "last_range_rescored"):
        assert getattr(mem, name) is None
    for name in ("uncertified_count", "grouped_uncertified_count", "scoped_uncertified_count",
                 "group_scoped_uncertified_count", "clip_uncertified_count"):
        assert getattr(mem, name) == 0


# ---- the scope coercion -----------------------------------------------------------------------------------------------
def test_scopes_with_a_count():
    mem = _memory()
    one = mem._scopes((3, 9), 4)
    assert one.dtype == torch.int64 and one.tolist() == [[3] * 4, [9] * 4]          # one pair stands for all
    pairs = [(0, 1), (2, 3), (4, 5)]
    assert mem._scopes(pairs, 3).tolist() == [[0, 2, 4], [1, 3, 5]]
    t = torch.tensor(pairs, dtype=torch.int64)
    got = mem._scopes(t, 3)
    assert got.tolist() == [[0, 2, 4], [1, 3, 5]] and got.is_contiguous() and got.dtype == torch.int64
    assert mem._scopes([(5, 6), (7, 8)], 2).tolist() == [[5, 7], [6, 8]]             # two pairs, not one pair of pairs
    for wrong in (pairs, t):
        with pytest.raises(ValueError, match="3 scopes for 2"):
            mem._scopes(wrong, 2)
    with pytest.raises(ValueError, match="pair"):
        mem._scopes([(0, 1), (2, 3, 4), (5, 6)], 3)
    for bad in (t.double(), t.to(torch.int32), t.reshape(-1), t.t().contiguous()):
        with pytest.raises(ValueError, match="int64"):
            mem._scopes(bad, 3)


def test_scopes_without_a_count():
    mem = _memory()
    assert mem._scopes((3, 9)).tolist() == [[3], [9]]                                # one pair: no broadcast
    assert mem._scopes([(0, 1), (2, 3), (4, 5)]).tolist() == [[0, 2, 4], [1, 3, 5]]
    assert mem._scopes(torch.tensor([[0, 1], [2, 3]], dtype=torch.int64)).tolist() == [[0, 2], [1, 3]]
    for empty in ([], torch.zeros((0, 2), dtype=torch.int64)):
        with pytest.raises(ValueError, match="scopes"):
            mem._scopes(empty)
    with pytest.raises(ValueError, match="pair"):
        mem._scopes([(0, 1, 2)])
    with pytest.raises(ValueError, match="int64"):
        mem._scopes(torch.zeros((2, 2)))


# ---- the column coercion ----------------------------------------------------------------------------------------------
def test_int64_column():
    mem = _memory()
    col, known = mem._int64_column(7, 3, "tags")
    assert col.dtype == torch.int64 and col.tolist() == [7, 7, 7] and known == [7]
    col, known = mem._int64_column([4, 5, 6], 3, "tags")
    assert col.dtype == torch.int64 and col.tolist() == [4, 5, 6] and known == [4, 5, 6]
    col, known = mem._int64_column(torch.tensor(9), 2, "tags")                       # 0-dim: one value for every row
    assert col.tolist() == [9, 9] and known == [9]
    col, known = mem._int64_column(torch.tensor([[1, 2], [3, 4]], dtype=torch.int32), 4, "tags")
    assert col.dtype == torch.int64 and col.tolist() == [1, 2, 3, 4] and known is None and col.is_contiguous()
    for value in ([1, 2], (1, 2), torch.tensor([1, 2])):
        with pytest.raises(ValueError, match="2 tags for 3 rows"):
            mem._int64_column(value, 3, "tags")
    with pytest.raises(ValueError, match="2 group keys for 3 rows"):
        mem._group_keys_for(3, [1, 2])
    assert mem._tags_for(3, [1, 2, 3]).tolist() == [1, 2, 3] and mem._tags_for(3, None) is None


def test_group_keys_keep_their_bookkeeping():
    mem = _memory()
    mem._next_group_key, mem._last_keys_dev = 0, None
    assert mem._group_keys_for(2, 5).tolist() == [5, 5] and mem._next_group_key == 6 and mem._last_keys_dev is None
    assert mem._group_keys_for(2, [9, 3]).tolist() == [9, 3] and mem._next_group_key == 10
    dev = torch.tensor([40, 41])
    assert mem._group_keys_for(2, dev).tolist() == [40, 41] and mem._next_group_key == 10    # not read on the host ...
    assert mem._last_keys_dev.tolist() == [40, 41]
    assert mem._group_keys_for(2, None).tolist() == [42, 42] and mem._last_keys_dev is None   # ... until a new group
    assert mem.new_group_key() == 43


def test_int64_cell():
    mem = _memory()
    assert mem._int64_cell(5).tolist() == [5] and mem._int64_cell(5).dtype == torch.int64
    assert mem._int64_cell(torch.tensor([8, 9], dtype=torch.int32)).tolist() == [8]
    assert mem._int64_cell(torch.tensor(4)).tolist() == [4]
