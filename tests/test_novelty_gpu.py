"""GPU: the novelty-gated append (vm_memory_append_novel) against statement (A) of tests/novelty_ref.py,
bit for bit: keep, row_of and the count of every call, and afterwards the memory itself - rows, tags, group keys, and
the answers of topk / topk_grouped / topk_scoped against the same calls on a memory built with plain ``append`` of the
kept rows (which covers norms and group ordinals without reading private columns)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import novelty_ref as N
from tests.support import from_bits

pytestmark = pytest.mark.gpu

SEQUENCE = (16, 17, 1, 300, 16, 250, 600)
SHAPES = [("f16", 768), ("bf16", 1024)]
KINDS = ["plain", "grouped", "tagged", "tagged_grouped"]


def _memory(kind, cap, D, dtype, ring=False):
    from vidmem.memory import EmbeddingMemory
    return EmbeddingMemory(cap, D, dtype, ring=ring, grouped="grouped" in kind, tagged="tagged" in kind)


def _gated(mem, batch_t, tau, known=None, group=None, tag=None):
    """One vm_memory_append_novel through the capturable form, then the host mirror brought in line."""
    keep, row_of, count = mem.enqueue_append_novel(batch_t, tau, known=known, group=group, tag=tag)
    out = keep.cpu().numpy().astype(bool), row_of.cpu().numpy().copy(), int(count.item())
    mem.sync()
    return out


def _assert_same_memory(mem, model, kind, dtype, queries):
    """``mem`` (gated on the device) against a memory built by plain appends of the model's rows, keys and tags."""
    ref = _memory(kind, mem.capacity, mem.dim, dtype, ring=mem.ring)
    step = max(1, min(mem.capacity, 4096))
    for lo in range(0, model.total, step):
        kw = {}
        if ref.grouped:
            kw["group"] = torch.from_numpy(model.keys[lo:lo + step].copy())
        if ref.tagged:
            kw["tag"] = torch.from_numpy(model.tags[lo:lo + step].copy())
        ref.append(from_bits(model.rows[lo:lo + step], dtype), **kw)
    assert len(mem) == len(ref) == model.total
    base, rows = mem.rows_host()
    base_r, rows_r = ref.rows_host()
    assert base == base_r and np.array_equal(rows, rows_r) and np.array_equal(rows, model.rows[base:])
    if mem.tagged:
        assert np.array_equal(mem.tags_host(), ref.tags_host())
        assert np.array_equal(mem.tags_host(), model.tags[base:])
    if mem.grouped:
        assert np.array_equal(mem.group_keys_host(), ref.group_keys_host())
        assert np.array_equal(mem.group_keys_host(), model.keys[base:])
    q = from_bits(queries, dtype)
    for a, b in zip(mem.topk(q, 10), ref.topk(q, 10)):
        assert torch.equal(a, b)
    if mem.grouped:
        for a, b in zip(mem.topk_grouped(q, 5), ref.topk_grouped(q, 5)):
            assert torch.equal(a, b)
    if mem.tagged:
        from vidmem.memory import SCOPE_ALL
        mid = int(np.median(model.tags[base:])) if model.total > base else 0
        for scope in (SCOPE_ALL, (0, mid)):
            for a, b in zip(mem.topk_scoped(q, 7, scope), ref.topk_scoped(q, 7, scope)):
                assert torch.equal(a, b)
    ref.close()


def _in_band(keep):
    """The condition on the inputs: the REFERENCE keeps between 5 % and 95 % of a batch of 16 rows or more."""
    if keep.size >= 16:
        assert 0.05 <= keep.mean() <= 0.95, keep.mean()


@pytest.mark.parametrize("sigma,tau", [(0.01, 0.9), (0.02, 0.7)])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype,D", SHAPES)
def test_recipe_sequence(dtype, D, kind, sigma, tau):
    from vidmem.memory import make_tag
    x = N.clip(1200, 300, D, sigma, dtype)
    mem = _memory(kind, 2048, D, dtype)
    model = N.GatedMemory(D, dtype)
    off = 0
    for step, B in enumerate(SEQUENCE):
        batch = x[off:off + B]
        idx = np.arange(off, off + B, dtype=np.int64)
        keys = idx // 16 if "grouped" in kind else None           # runs of 16 frames: groups continue across calls
        tags = np.array([make_tag(0, int(i) * 33) for i in idx], np.int64) if "tagged" in kind else None
        bt = from_bits(batch, dtype)
        want_ks, want_kr = model.known(batch)
        if mem.searchable == 0:
            known = None
        elif step % 2:                                            # column 0 of a top-10 result, passed in place
            s, r = mem.topk(bt, 10)
            assert s.stride(0) == 10
            known = (s, r)
            got_ks, got_kr = s[:, 0], r[:, 0]
        else:
            s, r = mem.topk(bt, 1)
            known = (s, r)
            got_ks, got_kr = s[:, 0], r[:, 0]
        if known is not None:
            assert np.array_equal(got_kr.cpu().numpy(), want_kr)
            assert np.array_equal(got_ks.cpu().numpy(), want_ks)
        want_keep, want_row_of = model.append_novel(batch, tau, known=(want_ks, want_kr), tags=tags, keys=keys)
        _in_band(want_keep)
        keep, row_of, count = _gated(mem, bt, tau, known=known,
                                     group=None if keys is None else torch.from_numpy(keys).cuda(),
                                     tag=None if tags is None else torch.from_numpy(tags).cuda())
        assert np.array_equal(keep, want_keep), (step, B)
        assert np.array_equal(row_of, want_row_of), (step, B)
        assert count == int(want_keep.sum()) and len(mem) == model.total
        off += B
    _assert_same_memory(mem, model, kind, dtype, x[[0, 5, 40, 333, 700, 1199]])


@pytest.mark.parametrize("dtype,D,B", [("f16", 768, 2048), ("bf16", 1024, 2048), ("f16", 768, 4096)])
def test_single_large_batch_into_an_empty_memory(dtype, D, B):
    x = N.clip(B, B // 4, D, 0.01, dtype)
    want_keep, want_row_of = N.gate(x, 0.9, dtype, 0)
    _in_band(want_keep)
    mem = _memory("plain", B, D, dtype)
    keep, row_of, count = _gated(mem, from_bits(x, dtype), 0.9)
    assert np.array_equal(keep, want_keep) and np.array_equal(row_of, want_row_of)
    assert count == int(want_keep.sum()) == len(mem)
    model = N.GatedMemory(D, dtype)
    model.rows = x[want_keep]
    model.tags = np.zeros(model.total, np.int64)
    model.keys = np.zeros(model.total, np.int64)
    _assert_same_memory(mem, model, "plain", dtype, x[[0, 1, B // 2, B - 1]])


def test_more_than_4096_rows_per_call_is_refused():
    from vidmem import _lib
    mem = _memory("plain", 8192, 128, "f16")
    rows = torch.zeros((4097, 128), dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError, match="4096"):
        mem.enqueue_append_novel(rows, 0.5)
    sc = mem.prepare_append_novel(4096)
    rc = mem.L.vm_memory_append_novel(mem.handle, C.c_void_p(rows.data_ptr()), 4097, 0.5, None, None, 1, None, None,
                                      None, None, None, C.c_void_p(sc.ws.data_ptr()), sc.ws.numel(),
                                      _lib.current_stream_ptr())
    assert rc == _lib.VM_ERR_UNSUPPORTED
    assert mem.L.vm_novelty_workspace_bytes(mem.handle, 4097) == 0
    # one of known_scores / known_rows without the other, NaN, columns the memory does not have
    one = torch.zeros(4, dtype=torch.float64, device="cuda")
    args = lambda **kw: [mem.handle, C.c_void_p(rows.data_ptr()), 4, kw.get("tau", 0.5),
                         C.c_void_p(kw.get("ks", 0)), C.c_void_p(kw.get("kr", 0)), 1, C.c_void_p(kw.get("tags", 0)),
                         C.c_void_p(kw.get("keys", 0)), None, None, None, C.c_void_p(sc.ws.data_ptr()), sc.ws.numel(),
                         _lib.current_stream_ptr()]
    assert mem.L.vm_memory_append_novel(*args(ks=one.data_ptr())) == _lib.VM_ERR_INVALID
    assert mem.L.vm_memory_append_novel(*args(kr=one.data_ptr())) == _lib.VM_ERR_INVALID
    assert mem.L.vm_memory_append_novel(*args(tau=float("nan"))) == _lib.VM_ERR_INVALID
    assert mem.L.vm_memory_append_novel(*args(tags=one.data_ptr())) == _lib.VM_ERR_INVALID
    assert mem.L.vm_memory_append_novel(*args(keys=one.data_ptr())) == _lib.VM_ERR_INVALID
    assert mem.sync() == 0
    # B = 0: a no-op that writes the count
    cnt = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    a = args()
    a[2], a[11] = 0, C.c_void_p(cnt.data_ptr())
    assert mem.L.vm_memory_append_novel(*a) == _lib.VM_OK
    assert int(cnt.item()) == 0 and mem.sync() == 0


@pytest.mark.parametrize("dtype,D", SHAPES)
def test_threshold_planted_on_a_score(dtype, D):
    """``>`` is strict: tau = the exact fp64 cosine of a pair keeps both rows, the next double below drops the second;
    the same for a known_score."""
    from oracle import cref
    x = N.clip(64, 8, D, 0.01, dtype, seed=11)
    m = cref.cosine_matrix(x, x, dtype=dtype)
    j = int(np.argmax(m[0, 1:])) + 1
    pair = np.stack([x[0], x[j]])
    tau = float(m[0, j])
    assert 0.5 < tau < 1.0
    for t, want in ((tau, [True, True]), (float(np.nextafter(tau, -np.inf)), [True, False])):
        mem = _memory("plain", 16, D, dtype)
        keep, row_of, count = _gated(mem, from_bits(pair, dtype), t)
        assert keep.tolist() == want and count == sum(want)
        assert row_of.tolist() == ([0, 1] if want[1] else [0, 0])
        assert np.array_equal(keep, N.gate(pair, t, dtype, 0)[0])
    # a known score exactly at the threshold keeps the row; one ulp above it drops it onto the known row
    ks = torch.tensor([tau], dtype=torch.float64, device="cuda")
    kr = torch.tensor([5], dtype=torch.int64, device="cuda")
    for t, want in ((tau, True), (float(np.nextafter(tau, -np.inf)), False)):
        mem = _memory("plain", 16, D, dtype, ring=True)
        mem.append(from_bits(x[8:16], dtype))
        keep, row_of, count = _gated(mem, from_bits(x[:1], dtype), t, known=(ks, kr))
        assert keep.tolist() == [want] and row_of.tolist() == [8 if want else 5] and count == int(want)
        assert len(mem) == 8 + int(want)


def test_duplicates_zero_rows_and_a_batch_that_keeps_nothing():
    dtype, D = "f16", 768
    x = N.clip(40, 40, D, 0.0, dtype, seed=3)            # 40 runs, sigma 0: frames of one run are exact duplicates
    rows = [x[0]]
    for r in x[1:]:
        if not any(np.array_equal(r, q) for q in rows):
            rows.append(r)
    u = np.stack(rows[:6])                               # six distinct directions
    zero = np.zeros((1, D), np.uint16)
    batch = np.concatenate([u[:2], u[1:2], zero, u[1:2], u[2:3], u[1:2], zero, u[1:2]])
    want_keep, want_row_of = N.gate(batch, 0.5, dtype, 3)
    assert want_keep.tolist() == [True, True, False, True, False, True, False, True, False]
    assert want_row_of.tolist() == [3, 4, 4, 5, 4, 6, 4, 7, 4]       # every duplicate names the first one's new id
    mem = _memory("grouped", 64, D, dtype)
    mem.append(from_bits(u[3:6], dtype), group=[7, 7, 9])
    keep, row_of, count = _gated(mem, from_bits(batch, dtype), 0.5, group=torch.full((9,), 9, dtype=torch.int64).cuda())
    assert np.array_equal(keep, want_keep) and np.array_equal(row_of, want_row_of) and count == 5
    # a batch that keeps nothing: counter, columns and group state untouched ...
    before = (mem.rows_host()[1].copy(), mem.group_keys_host().copy())
    s, r = mem.topk(from_bits(u[:3], dtype), 1)
    keep, row_of, count = _gated(mem, from_bits(u[:3], dtype), 0.5, known=(s, r),
                                 group=torch.full((3,), 11, dtype=torch.int64).cuda())
    assert keep.tolist() == [False] * 3 and count == 0 and len(mem) == 8
    assert row_of.tolist() == [3, 4, 6]
    assert np.array_equal(mem.rows_host()[1], before[0]) and np.array_equal(mem.group_keys_host(), before[1])
    # ... so a grouped append with the previous key still continues the open group (key 9: rows 2 and 3..7 and the new one)
    mem.append(from_bits(u[3:4], dtype), group=9)
    model = N.GatedMemory(D, dtype)
    model.rows = np.concatenate([u[3:6], batch[want_keep], u[3:4]])
    model.keys = np.array([7, 7, 9, 9, 9, 9, 9, 9, 9], np.int64)
    model.tags = np.zeros(9, np.int64)
    _assert_same_memory(mem, model, "grouped", dtype, u)
    sg, rg, kg = mem.topk_grouped(from_bits(u[3:4], dtype), 3)
    assert kg[0, 0].item() in (7, 9) and len(set(kg[0].tolist()) - {-1}) == 2       # two groups in all


@pytest.mark.parametrize("kind", ["plain", "tagged_grouped"])
def test_threshold_2_is_plain_append_and_minus_2_keeps_one_row(kind):
    dtype, D = "bf16", 1024
    x = N.clip(100, 25, D, 0.01, dtype, seed=9)
    mem = _memory(kind, 256, D, dtype)
    model = N.GatedMemory(D, dtype)
    kw = {}
    if "grouped" in kind:
        kw = {"group": torch.arange(100).cuda() // 7, "tag": torch.arange(100).cuda() * 5}
    for lo, hi in ((0, 37), (37, 100)):
        sub = {k: v[lo:hi] for k, v in kw.items()}
        keep, row_of, count = _gated(mem, from_bits(x[lo:hi], dtype), 2.0, **sub)
        assert keep.all() and count == hi - lo and row_of.tolist() == list(range(lo, hi))
    model.rows = x
    model.keys = np.arange(100, dtype=np.int64) // 7 if kw else -1 - np.arange(100, dtype=np.int64)
    model.tags = np.arange(100, dtype=np.int64) * 5
    _assert_same_memory(mem, model, kind, dtype, x[[0, 50, 99]])       # bit-identical to the plain appends
    empty = _memory(kind, 256, D, dtype)
    keep, row_of, count = _gated(empty, from_bits(x, dtype), -2.0)
    assert keep.tolist() == [True] + [False] * 99 and count == 1 and (row_of == 0).all() and len(empty) == 1


def test_ring_that_wraps_inside_the_call_and_an_overwritten_known_row():
    dtype, D, cap = "f16", 768, 64
    x = N.clip(1500, 750, D, 0.01, dtype, seed=21)
    mem = _memory("tagged", cap, D, dtype, ring=True)
    model = N.GatedMemory(D, dtype, capacity=cap)
    off = 0
    for B in (40, 60, 64, 50) + (64,) * 20:         # the ring wraps inside several of the calls
        batch = x[off:off + B]
        tags = np.arange(off, off + B, dtype=np.int64)
        known = model.known(batch)                  # describes the memory BEFORE the call, as the definition says
        bt = from_bits(batch, dtype)
        dev_known = mem.topk(bt, 1) if mem.searchable else None
        want_keep, want_row_of = model.append_novel(batch, 0.9, known=known, tags=tags)
        _in_band(want_keep)
        keep, row_of, count = _gated(mem, bt, 0.9, known=dev_known, tag=torch.from_numpy(tags).cuda())
        assert np.array_equal(keep, want_keep) and np.array_equal(row_of, want_row_of) and count == want_keep.sum()
        off += B
    assert model.total > 2 * cap
    _assert_same_memory(mem, model, "tagged", dtype, x[[0, 100, 1499]])
    # a known row that the call itself overwrites: row_of names it all the same (the definition as written)
    base = model.total - cap
    batch = np.concatenate([x[:cap - 1], model.rows[base:base + 1]])     # cap - 1 new rows, then a copy of the oldest
    known = model.known(batch)
    assert known[1][-1] == base and known[0][-1] > 0.99
    want_keep, want_row_of = model.append_novel(batch, 0.9, known=known)
    assert not want_keep[-1] and want_row_of[-1] == base and want_keep.sum() > 1
    bt = from_bits(batch, dtype)
    keep, row_of, count = _gated(mem, bt, 0.9, known=mem.topk(bt, 1))
    assert np.array_equal(keep, want_keep) and np.array_equal(row_of, want_row_of)
    assert len(mem) == model.total and base < model.total - cap          # ... and that row is gone now


def test_non_ring_capacity():
    from vidmem import _lib
    from vidmem.memory import _tensor_from_ptr
    dtype, D = "f16", 768
    x = N.clip(400, 400, D, 0.0, dtype, seed=4)      # sigma 0: a run is one vector; distinct runs are near-orthogonal
    distinct = np.unique(x, axis=0)[:40]
    assert distinct.shape[0] == 40
    mem = _memory("plain", 32, D, dtype)
    mem.append(from_bits(distinct[:10], dtype))
    with pytest.raises(_lib.VidmemError) as e:       # 10 + 23 > 32: refused on the worst case, whatever would be kept
        mem.enqueue_append_novel(from_bits(distinct[:23], dtype), 0.5)
    assert e.value.code == _lib.VM_ERR_NOMEM and mem.sync() == 10
    # a stale mirror (two enqueued calls without a sync between them) must still never write past the capacity
    keep1, _, c1 = mem.enqueue_append_novel(from_bits(distinct[10:30], dtype), 0.5)
    assert int(c1.item()) == 20
    keep2, _, c2 = mem.enqueue_append_novel(from_bits(distinct[20:40], dtype), 0.5)     # mirror still says 10
    assert mem.sync() == 32 and len(mem) == 32
    pad = _tensor_from_ptr(mem.L.vm_memory_rows(mem.handle), (64, D), torch.int16, mem.device)
    assert np.array_equal(pad[:30].cpu().numpy().view(np.uint16), distinct[:30])
    assert not pad[32:].any()                        # the padding rows behind the capacity were never written


def test_capture_topk_redo_and_gated_append_in_one_graph():
    """{topk, redo, enqueue_append_novel} captured once, replayed with rows, tags and keys rewritten in place; the ring
    wraps among the replays; then sync()."""
    from vidmem.memory import NoveltyScratch, TopkScratch
    dtype, D, cap, B, k = "f16", 768, 64, 32, 10
    x = N.clip(40 + 6 * B, 200, D, 0.01, dtype, seed=17)
    mem = _memory("tagged_grouped", cap, D, dtype, ring=True)
    model = N.GatedMemory(D, dtype, capacity=cap)
    seed_keys = np.arange(40, dtype=np.int64) // 8
    mem.append(from_bits(x[:40], dtype), group=torch.from_numpy(seed_keys), tag=torch.arange(40))
    model.rows, model.keys, model.tags = x[:40].copy(), seed_keys.copy(), np.arange(40, dtype=np.int64)
    rows_in = torch.zeros((B, D), dtype=torch.float16, device="cuda")
    tags_in = torch.zeros(B, dtype=torch.int64, device="cuda")
    keys_in = torch.zeros(B, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    tk, nv = TopkScratch.for_(mem, B, k), NoveltyScratch.for_(mem, B)

    def body():
        s, r = mem.topk(rows_in, k, scratch=tk)
        keep, row_of, count = mem.enqueue_append_novel(rows_in, 0.9, known=(s, r), group=keys_in, tag=tags_in,
                                                       scratch=nv)
        return s, r, keep, row_of, count

    with torch.cuda.stream(stream):
        warm = _memory("tagged_grouped", cap, D, dtype, ring=True)
        warm.append(from_bits(x[:4], dtype), group=0, tag=0)
        real = mem
        mem = warm
        body()
        mem = real
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            s, r, keep, row_of, count = body()
        mem.sync()
    assert len(mem) == 40
    off = 40
    for step in range(6):
        batch = x[off:off + B]
        tags = np.arange(off, off + B, dtype=np.int64) * 3
        keys = np.arange(off, off + B, dtype=np.int64) // 8
        want_ks, want_kr = model.known(batch)
        want_keep, want_row_of = model.append_novel(batch, 0.9, known=(want_ks, want_kr), tags=tags, keys=keys)
        _in_band(want_keep)
        with torch.cuda.stream(stream):
            rows_in.copy_(from_bits(batch, dtype))
            tags_in.copy_(torch.from_numpy(tags))
            keys_in.copy_(torch.from_numpy(keys))
            graph.replay()
        stream.synchronize()
        assert np.array_equal(s[:, 0].cpu().numpy(), want_ks) and np.array_equal(r[:, 0].cpu().numpy(), want_kr)
        assert np.array_equal(keep.cpu().numpy().astype(bool), want_keep), step
        assert np.array_equal(row_of.cpu().numpy(), want_row_of), step
        assert int(count.item()) == int(want_keep.sum())
        off += B
    assert model.total > cap and len(mem) == 40          # wrapped; the host mirror lags until sync()
    assert mem.sync() == model.total and len(mem.ids) == len(mem)
    _assert_same_memory(mem, model, "tagged_grouped", dtype, x[[3, 77, 200]])


def test_against_a_scope_against_none_and_the_eager_tables():
    from vidmem.memory import scope_of, make_tag
    dtype, D = "f16", 768
    x = N.clip(48, 12, D, 0.01, dtype, seed=8)
    mem = _memory("tagged", 512, D, dtype)
    want_keep, want_row_of = N.gate(x, 0.9, dtype, 0)
    _in_band(want_keep)
    n0 = int(want_keep.sum())
    ids = [f"a_{i}" for i in range(48)]
    nov = mem.append_novel(from_bits(x, dtype), 0.9, ids=ids, meta=[{"i": i} for i in range(48)],
                           tag=[make_tag(0, i) for i in range(48)])
    assert nov.kept == n0 == len(mem) == len(mem.ids)
    assert nov.keep.dtype == torch.bool and np.array_equal(nov.keep.cpu().numpy(), want_keep)
    assert np.array_equal(nov.row_of.cpu().numpy(), want_row_of)
    assert mem.ids == [ids[i] for i in np.nonzero(want_keep)[0]] and mem.meta_of(0) == {"i": 0}
    # the same frames again: nothing is new for the whole memory or for source 0 ...
    assert mem.append_novel(from_bits(x, dtype), 0.9, tag=make_tag(0, 99)).kept == 0
    assert mem.append_novel(from_bits(x, dtype), 0.9, against=scope_of(0), tag=make_tag(0, 99)).kept == 0
    # ... but they are new for source 1, although source 0 holds them
    nov1 = mem.append_novel(from_bits(x, dtype), 0.9, against=scope_of(1), tag=make_tag(1, 0))
    assert nov1.kept == n0 and np.array_equal(nov1.keep.cpu().numpy(), want_keep)
    assert np.array_equal(nov1.row_of.cpu().numpy(), N.gate(x, 0.9, dtype, n0)[1])
    assert len(mem) == 2 * n0 and (mem.tags_host()[n0:] == make_tag(1, 0)).all()
    # and a second time they are known to source 1 too
    assert mem.append_novel(from_bits(x, dtype), 0.9, against=scope_of(1), tag=make_tag(1, 1)).kept == 0
    # against=None: among the batch only, whatever is stored
    nov2 = mem.append_novel(from_bits(x, dtype), 0.9, against=None)
    assert nov2.kept == n0 and np.array_equal(nov2.row_of.cpu().numpy(), N.gate(x, 0.9, dtype, 2 * n0)[1])
    assert (mem.tags_host()[2 * n0:] == -(1 << 63)).all() and len(mem.ids) == 3 * n0 == len(mem)
