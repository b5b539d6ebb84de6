"""GPU: erase (vm_memory_erase_scoped / vm_memory_erase_rows, csrc/erase.hip) against tests/erase_ref.py.

Bar: after an erase the memory is, bit for bit, a fresh memory of the same kind that was appended the survivors: the row,
tag and key columns over every slot the memory ever used (the vacated ones read zero, as in the fresh memory), the row
count, ``new_row_of`` and the erased count; norms, reciprocal norms, group ordinals and the group state through the
searches, whose rows and fp64 scores must equal the C oracle's over the survivors bit for bit (tests/topk_ref.py,
group_ref.py, scope_ref.py).  2,000 rows in a capacity of 2,100 with the workspace for 256-row segments: eight segments.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import cref
from tests import erase_ref as E
from tests import group_ref as G
from tests import scope_ref as S
from tests.support import MS, TD, from_bits

pytestmark = pytest.mark.gpu

N, CAP, SEG = 2000, 2100, 256
SHAPES = [("f16", 128), ("bf16", 768)]
KINDS = ["plain", "tagged", "grouped", "tagged_grouped"]


@functools.lru_cache(maxsize=None)
def _data(dtype, D, n=N, seed=5):
    """(row bits [n, D], tags [n], keys [n], query bits [5, D]); shared by every test, never modified.  Tags: sources of
    250 rows, MS apart - strictly rising with the row id, so a row range is one scope.  Keys: runs of 7 rows whose key
    comes back every 40 runs, so that erasing what lies between two runs of one key makes them adjacent.  Row norms are
    spread over a factor of 16."""
    rng = np.random.default_rng(seed)
    scale = 2.0 ** rng.uniform(-2, 2, size=(n + 2, 1))             # norms over a factor of 16: a norm that moved to the
    x = torch.from_numpy((rng.standard_normal((n + 2, D)) * scale).astype(np.float32)).to(TD[dtype])     # wrong row shows
    bits = x.view(torch.int16).numpy().view(np.uint16)
    i = np.arange(n, dtype=np.int64)
    tags = ((i // 250) << 40) | ((i % 250) * MS)
    keys = (i // 7) % 40
    q = np.stack([bits[3], bits[n // 3], bits[n - 1], bits[n], bits[n + 1]])
    return bits[:n], tags, keys, q


def _memory(kind, cap, D, dtype, ring=False):
    from vidmem.memory import EmbeddingMemory
    return EmbeddingMemory(cap, D, dtype, ring=ring, grouped="grouped" in kind, tagged="tagged" in kind)


def _fill(mem, cols: E.Columns, dtype):
    kw = {}
    if mem.grouped:
        kw["group"] = torch.from_numpy(np.array(cols.keys))
    if mem.tagged:
        kw["tag"] = torch.from_numpy(np.array(cols.tags))
    if cols.rows.shape[0]:
        mem.append(from_bits(cols.rows, dtype), **kw)
    return mem


def _columns(kind, dtype, D):
    bits, tags, keys, _ = _data(dtype, D)
    return E.Columns(bits, tags if "tagged" in kind else None, keys if "grouped" in kind else None)


def _raw(mem, n):
    """The row, tag and key columns over slots [0, n), raw (slot order): vacated slots included."""
    from vidmem.memory import _tensor_from_ptr
    out = [_tensor_from_ptr(mem.L.vm_memory_rows(mem.handle), (n, mem.dim), torch.int16, mem.device).cpu().numpy()]
    if mem.tagged:
        out.append(_tensor_from_ptr(mem.L.vm_memory_tags(mem.handle), (n,), torch.int64, mem.device).cpu().numpy())
    if mem.grouped:
        out.append(_tensor_from_ptr(mem.L.vm_memory_group_keys(mem.handle), (n,), torch.int64, mem.device).cpu().numpy())
    return out


def _erase(mem, rows=None, scope=None):
    """One erase through the capturable form with 256-row segments, then the host mirror brought in line."""
    sc = mem.prepare_erase(SEG)
    n_old = len(mem)
    new_row_of, erased = mem.enqueue_erase(rows=rows, scope=scope, scratch=sc)
    out = new_row_of[:n_old].cpu().numpy().copy(), int(erased.item())
    mem.sync()
    return out


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def _check_searches(mem, cols: E.Columns, dtype, qbits, base=0):
    """topk / topk_grouped / topk_scoped of ``mem`` against the oracle over ``cols`` (the rows ``mem`` should hold)."""
    if cols.rows.shape[0] == 0:
        return
    q = from_bits(qbits, dtype)
    want_r, want_s = cref.cosine_topk(np.ascontiguousarray(qbits), np.ascontiguousarray(cols.rows), 10, dtype=dtype)
    s, r = mem.topk(q, 10)
    assert np.array_equal(r.cpu().numpy(), np.where(want_r >= 0, want_r + base, -1))
    assert _same_bits(s.cpu().numpy(), want_s), "top-k scores differ from the oracle (bit-exact bar)"
    if mem.grouped:
        want_r, want_s, want_k = G.grouped_topk(qbits, cols.rows, cols.keys, 10, dtype=dtype, base=base)
        s, r, k = mem.topk_grouped(q, 10)
        assert np.array_equal(r.cpu().numpy(), want_r) and np.array_equal(k.cpu().numpy(), want_k)
        assert _same_bits(s.cpu().numpy(), want_s)
    if mem.tagged:
        pool = [(int(np.median(cols.tags)), S.INT64_MAX), (S.INT64_MIN, S.INT64_MAX), (1 << 40, (3 << 40) - 1)]
        scopes = [pool[i % 3] for i in range(qbits.shape[0])]
        want_r, want_s = S.scoped_topk(qbits, cols.rows, cols.tags, scopes, 10, dtype=dtype, base=base)
        s, r = mem.topk_scoped(q, 10, scopes)
        assert np.array_equal(r.cpu().numpy(), want_r)
        assert _same_bits(s.cpu().numpy(), want_s)


def _check_against_fresh(mem, kind, dtype, model: E.ErasedModel, n_used, qbits):
    """``mem`` after the erase against a fresh memory that was appended the survivors, and against the oracle."""
    fresh = _fill(_memory(kind, mem.capacity, mem.dim, dtype, ring=mem.ring), model.cols, dtype)
    n_new = model.cols.rows.shape[0]
    assert len(mem) == len(fresh) == n_new
    for a, b in zip(_raw(mem, n_used), _raw(fresh, n_used)):
        assert np.array_equal(a, b)
    assert np.array_equal(_raw(mem, n_used)[0][:n_new].view(np.uint16), model.cols.rows)
    assert not _raw(mem, n_used)[0][n_new:].any()                 # forgetting means the bytes are gone
    if n_new:
        q = from_bits(qbits, dtype)
        mem.reset_uncertified()
        for a, b in zip(mem.topk(q, 10), fresh.topk(q, 10)):
            assert torch.equal(a, b)
        assert mem.uncertified_count == fresh.uncertified_count       # the fp32 scan (reciprocal norms) saw the same
        if mem.grouped:
            for a, b in zip(mem.topk_grouped(q, 10), fresh.topk_grouped(q, 10)):
                assert torch.equal(a, b)
    _check_searches(mem, model.cols, dtype, qbits)
    fresh.close()


# ---- 1. the drop patterns ---------------------------------------------------------------------------------------------
def _ranges(*rr):
    drop = np.zeros(N, bool)
    for a, b in rr:
        drop[a:b] = True
    return drop, list(rr)


def _pattern(name):
    """-> (drop mask, row ranges [a, b) when the pattern is a union of ranges - tagged memories then erase by scope)."""
    if name == "nothing":
        return np.zeros(N, bool), []
    if name == "everything":
        return _ranges((0, N))
    if name == "first_row":
        return _ranges((0, 1))
    if name == "last_row":
        return _ranges((N - 1, N))
    if name == "scope_of_700_inside_a_segment":        # the segments behind it copy directly
        return _ranges((300, 1000))
    if name == "random_half":                          # scratch branch first, direct later
        return np.random.default_rng(12).random(N) < 0.5, None
    if name == "all_but_one_row_of_every_segment":
        drop = np.ones(N, bool)
        drop[17::SEG] = False
        return drop, None
    if name == "one_row_of_the_last_segment":
        return _ranges((1900, 1901))
    if name == "three_disjoint_scopes":
        return _ranges((100, 150), (700, 1300), (1990, N))
    raise KeyError(name)


PATTERNS = ["nothing", "everything", "first_row", "last_row", "scope_of_700_inside_a_segment", "random_half",
            "all_but_one_row_of_every_segment", "one_row_of_the_last_segment", "three_disjoint_scopes"]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype,D", SHAPES)
def test_drop_patterns(dtype, D, kind, pattern):
    cols = _columns(kind, dtype, D)
    qbits = _data(dtype, D)[3]
    drop, ranges = _pattern(pattern)
    mem = _fill(_memory(kind, CAP, D, dtype), cols, dtype)
    assert mem.L.vm_memory_erase_workspace_bytes(mem.handle, SEG) < mem.L.vm_memory_erase_workspace_bytes(mem.handle, 0)
    if mem.tagged and ranges is not None:
        scopes = [(int(cols.tags[a]), int(cols.tags[b - 1])) for a, b in ranges] or [(5, 3)]     # lo > hi: nothing
        new_row_of, erased = _erase(mem, scope=scopes)
    else:
        ids = np.nonzero(drop)[0]
        new_row_of, erased = _erase(mem, rows=torch.from_numpy(ids) if ids.size else torch.tensor([-1, N, 1 << 40]))
    model = E.erase(cols, drop)
    assert erased == model.count and np.array_equal(new_row_of, model.new_row_of)
    _check_against_fresh(mem, kind, dtype, model, N, qbits)
    mem.close()


# ---- 2. groups ----------------------------------------------------------------------------------------------------------
def test_groups_merge_when_the_group_between_them_goes():
    dtype, D = "f16", 128
    bits, _, _, _ = _data(dtype, D)
    keys = np.array([4] * 10 + [9] * 10 + [4] * 10, np.int64)                 # A B A
    cols = E.Columns(bits[:30], None, keys)
    mem = _fill(_memory("grouped", 64, D, dtype), cols, dtype)
    q = from_bits(bits[[2, 25]], dtype)
    assert set(mem.topk_grouped(q, 3)[2][0].tolist()) == {4, 9}
    assert mem.topk_grouped(q, 3)[2][0].tolist().count(4) == 2                # two groups with key 4
    new_row_of, erased = _erase(mem, rows=list(range(10, 20)))
    model = E.erase(cols, E.mask_of_rows(30, range(10, 20)))
    assert erased == 10 and np.array_equal(new_row_of, model.new_row_of) and model.state == (1, 4, 1)
    s, r, k = mem.topk_grouped(q, 3)
    assert k.tolist() == [[4, -1, -1], [4, -1, -1]] and r.tolist() == [[2, -1, -1], [15, -1, -1]]       # one group A
    _check_against_fresh(mem, "grouped", dtype, model, 30, bits[[2, 25, 40]])


def test_erasing_the_last_row_leaves_the_group_before_it_open():
    dtype, D = "f16", 128
    bits, _, _, _ = _data(dtype, D)
    cols = E.Columns(bits[:6], None, np.array([1, 1, 1, 1, 1, 2], np.int64))
    mem = _fill(_memory("grouped", 64, D, dtype), cols, dtype)
    new_row_of, erased = _erase(mem, rows=[5])
    assert erased == 1 and new_row_of.tolist() == [0, 1, 2, 3, 4, -1]
    mem.append(from_bits(bits[6:9], dtype), group=torch.tensor([1, 1, 3]))           # continues group 1, then opens group 3
    want = E.Columns(np.concatenate([bits[:5], bits[6:9]]), None, np.array([1] * 7 + [3], np.int64))
    fresh = _fill(_memory("grouped", 64, D, dtype), want, dtype)
    q = from_bits(bits[[0, 7, 8]], dtype)
    got = mem.topk_grouped(q, 4)
    for a, b in zip(got, fresh.topk_grouped(q, 4)):
        assert torch.equal(a, b)
    assert got[2].tolist()[0][:2] in ([1, 3], [3, 1]) and got[2].tolist()[0][2:] == [-1, -1]          # two groups in all
    _check_searches(mem, want, dtype, bits[[0, 7, 8]])


# ---- 3. the rows form ---------------------------------------------------------------------------------------------------
def test_rows_form_takes_a_padded_topk_result_and_an_empty_list():
    from vidmem import _lib
    dtype, D = "bf16", 768
    cols = _columns("tagged_grouped", dtype, D)
    qbits = _data(dtype, D)[3]
    mem = _fill(_memory("tagged_grouped", CAP, D, dtype), cols, dtype)
    s, r = mem.topk(from_bits(qbits, dtype), 10, min_score=0.1)
    assert r.shape == (5, 10) and (r == -1).any() and (r >= 0).any()          # a padded result
    ids = torch.cat([r, r[:2], torch.full((1, 10), N + 7, dtype=torch.int64, device="cuda")])       # duplicates, past the end
    out = mem.erase(rows=ids)
    model = E.erase(cols, E.mask_of_rows(N, ids.cpu().numpy()))
    assert out.count == model.count > 0 and np.array_equal(out.new_row_of.cpu().numpy(), model.new_row_of)
    _check_against_fresh(mem, "tagged_grouped", dtype, model, N, qbits)
    # n = 0: a no-op that writes a zero count
    n_before = len(mem)
    cnt = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    sc = mem.prepare_erase(SEG)
    rc = mem.L.vm_memory_erase_rows(mem.handle, None, 0, None, C.c_void_p(cnt.data_ptr()), C.c_void_p(sc.ws.data_ptr()),
                                    sc.ws.numel(), _lib.current_stream_ptr())
    assert rc == _lib.VM_OK and int(cnt.item()) == 0 and mem.sync() == n_before
    assert mem.erase(rows=[]).count == 0 and len(mem) == n_before
    # refusals: a scope on an untagged memory, no scope, a workspace without 256 rows of scratch
    plain = _fill(_memory("plain", 64, 128, "f16"), E.Columns(_data("f16", 128)[0][:8], None, None), "f16")
    with pytest.raises(ValueError, match="tagged"):
        plain.erase(scope=(0, 5))
    psc = plain.prepare_erase(0)
    one = torch.zeros(2, dtype=torch.int64, device="cuda")
    args = [plain.handle, C.c_void_p(one.data_ptr()), C.c_void_p(one.data_ptr()), 1, None, None,
            C.c_void_p(psc.ws.data_ptr()), psc.ws.numel(), _lib.current_stream_ptr()]
    assert plain.L.vm_memory_erase_scoped(*args) == _lib.VM_ERR_INVALID
    args[0], args[3] = mem.handle, 0
    assert mem.L.vm_memory_erase_scoped(*args) == _lib.VM_ERR_INVALID
    small = plain.L.vm_memory_erase_workspace_bytes(plain.handle, 256) - 256 * (2 * 128 + 28) + 255 * (2 * 128 + 28)
    assert plain.L.vm_memory_erase_rows(plain.handle, C.c_void_p(one.data_ptr()), 2, None, None,
                                        C.c_void_p(psc.ws.data_ptr()), small, _lib.current_stream_ptr()) == _lib.VM_ERR_NOMEM
    assert plain.sync() == 8


# ---- 4. capacity --------------------------------------------------------------------------------------------------------
def test_erase_reclaims_the_capacity_of_a_full_memory():
    from vidmem import _lib
    from vidmem.memory import make_tag, scope_of
    dtype, D, cap = "f16", 128, 512
    bits, _, _, qbits = _data(dtype, D)
    tags = np.array([make_tag(i // 100, (i % 100) * MS) for i in range(cap)], np.int64)
    cols = E.Columns(bits[:cap], tags, None)
    mem = _fill(_memory("tagged", cap, D, dtype), cols, dtype)
    with pytest.raises(_lib.VidmemError) as e:
        mem.append(from_bits(bits[cap:cap + 1], dtype), tag=make_tag(9, 0))
    assert e.value.code == _lib.VM_ERR_NOMEM
    out = mem.erase(scope=[scope_of(1), scope_of(2), scope_of(4)])           # 300 rows
    assert out.count == 300 and len(mem) == cap - 300
    new_tags = np.array([make_tag(9, i * MS) for i in range(300)], np.int64)
    assert mem.append(from_bits(bits[1000:1300], dtype), tag=torch.from_numpy(new_tags)) == cap - 300
    assert len(mem) == cap
    model = E.erase(cols, E.mask_of_scopes(tags, [scope_of(1), scope_of(2), scope_of(4)]))
    want = E.Columns(np.concatenate([model.cols.rows, bits[1000:1300]]), np.concatenate([model.cols.tags, new_tags]), None)
    assert np.array_equal(mem.rows_host()[1], want.rows) and np.array_equal(mem.tags_host(), want.tags)
    _check_searches(mem, want, dtype, np.stack([bits[3], bits[450], bits[1000], bits[1299], qbits[4]]))


# ---- 5. rings -----------------------------------------------------------------------------------------------------------
def test_ring_below_its_capacity_erases_and_then_wraps():
    dtype, D, cap = "f16", 128, 256
    bits, _, _, _ = _data(dtype, D)
    tags = np.arange(400, dtype=np.int64) * 3
    mem = _memory("tagged", cap, D, dtype, ring=True)
    mem.append(from_bits(bits[:200], dtype), tag=torch.from_numpy(tags[:200]))
    drop = E.mask_of_rows(200, range(40, 90))
    new_row_of, erased = _erase(mem, rows=torch.arange(40, 90))
    model = E.erase(E.Columns(bits[:200], tags[:200], None), drop)
    assert erased == 50 and np.array_equal(new_row_of, model.new_row_of) and len(mem) == 150
    mem.append(from_bits(bits[200:400], dtype), tag=torch.from_numpy(tags[200:400]))           # 350 rows: the ring wraps
    assert len(mem) == 350 and mem.searchable == cap
    all_rows = np.concatenate([model.cols.rows, bits[200:400]])
    all_tags = np.concatenate([model.cols.tags, tags[200:400]])
    base, host = mem.rows_host()
    assert base == 94 and np.array_equal(host, all_rows[94:]) and np.array_equal(mem.tags_host(), all_tags[94:])
    _check_searches(mem, E.Columns(all_rows[94:], all_tags[94:], None), dtype, bits[[0, 100, 250, 399, 1000]], base=94)


def test_wrapped_ring_is_refused_and_the_device_guards_a_stale_mirror():
    from vidmem import _lib
    dtype, D, cap = "f16", 128, 64
    bits, _, _, _ = _data(dtype, D)
    mem = _memory("tagged_grouped", cap, D, dtype, ring=True)
    mem.append(from_bits(bits[:60], dtype), tag=torch.arange(60), group=torch.arange(60) // 4)
    # 20 more rows through the gated append, which does not advance the host mirror: the device wraps, the mirror says 60
    mem.enqueue_append_novel(from_bits(bits[60:80], dtype), 2.0, tag=torch.arange(60, 80).cuda(),
                             group=(torch.arange(60, 80) // 4).cuda())
    assert len(mem) == 60
    before = _raw(mem, cap)
    sc = mem.prepare_erase(SEG)
    sc.new_row_of.fill_(-5)
    new_row_of, erased = mem.enqueue_erase(rows=[1, 2, 3], scratch=sc)
    assert int(erased.item()) == -1 and (new_row_of == -5).all()             # the device guard: nothing touched
    assert mem.sync() == 80
    for a, b in zip(before, _raw(mem, cap)):
        assert np.array_equal(a, b)
    # with the mirror current the call is refused on the host
    for kw in ({"rows": [1, 2, 3]}, {"scope": (0, 10)}):
        with pytest.raises(_lib.VidmemError) as e:
            mem.erase(**kw)
        assert e.value.code == _lib.VM_ERR_UNSUPPORTED
    assert mem.sync() == 80
    for a, b in zip(before, _raw(mem, cap)):
        assert np.array_equal(a, b)
    want = E.Columns(bits[16:80], np.arange(16, 80, dtype=np.int64), np.arange(16, 80, dtype=np.int64) // 4)
    _check_searches(mem, want, dtype, bits[[20, 50, 79]], base=16)


# ---- 6. graph replay ----------------------------------------------------------------------------------------------------
def test_capture_append_erase_older_than_and_scoped_search_in_one_graph():
    from vidmem.memory import EraseScratch, make_tag
    dtype, D, cap, B, Q, k = "f16", 128, 512, 64, 4, 5
    bits, _, _, _ = _data(dtype, D)
    mem = _memory("tagged", cap, D, dtype)
    t_of = lambda i: make_tag(0, int(i) * MS)
    model = E.Columns(bits[:100], np.array([t_of(i) for i in range(100)], np.int64), None)
    _fill(mem, model, dtype)
    rows_in = torch.zeros((B, D), dtype=TD[dtype], device="cuda")
    tags_in = torch.zeros(B, dtype=torch.int64, device="cuda")
    older = torch.zeros((1, 2), dtype=torch.int64, device="cuda")             # [start of source 0, T]
    q_in = torch.zeros((Q, D), dtype=TD[dtype], device="cuda")
    window = torch.zeros((Q, 2), dtype=torch.int64, device="cuda")
    es = EraseScratch.for_(mem, SEG)
    mem.prepare_topk_scoped(Q, k)
    warm = _fill(_memory("tagged", cap, D, dtype), model, dtype)             # load every kernel before the capture
    warm.enqueue_erase(scope=older)
    warm.topk_scoped(q_in, k, window)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            mem.append(rows_in, tag=tags_in)
            new_row_of, erased = mem.enqueue_erase(scope=older, scratch=es)
            out_s, out_r = mem.topk_scoped(q_in, k, window)
    torch.cuda.current_stream().wait_stream(s)
    assert mem.sync() == 100                                                   # the capture ran nothing
    for rep in range(3):
        lo = 100 + rep * B
        new_tags = np.array([t_of(i) for i in range(lo, lo + B)], np.int64)
        T = t_of(30 + 70 * rep)                                               # 31, 70, 70 rows older than T
        windows = [(T + 1, S.INT64_MAX), (t_of(lo), t_of(lo + B)), (0, T), (S.INT64_MIN, S.INT64_MAX)]
        qb = np.stack([bits[50 + 70 * rep], bits[lo + 1], bits[3], bits[lo + B - 1]])
        rows_in.copy_(from_bits(bits[lo:lo + B], dtype))
        tags_in.copy_(torch.from_numpy(new_tags))
        older.copy_(torch.tensor([[t_of(0), T]]))
        q_in.copy_(from_bits(qb, dtype))
        window.copy_(torch.tensor(windows, dtype=torch.int64))
        graph.replay()
        torch.cuda.synchronize()
        appended = E.Columns(np.concatenate([model.rows, bits[lo:lo + B]]), np.concatenate([model.tags, new_tags]), None)
        want = E.erase(appended, E.mask_of_scopes(appended.tags, [(t_of(0), T)]))
        assert want.count == (31, 70, 70)[rep]
        assert int(erased.item()) == want.count
        assert np.array_equal(new_row_of[:appended.rows.shape[0]].cpu().numpy(), want.new_row_of)
        model = want.cols
        assert mem.sync() == model.rows.shape[0]
        assert np.array_equal(mem.rows_host()[1], model.rows) and np.array_equal(mem.tags_host(), model.tags)
        want_r, want_s = S.scoped_topk(qb, model.rows, model.tags, windows, k, dtype=dtype)
        assert np.array_equal(out_r.cpu().numpy(), want_r) and _same_bits(out_s.cpu().numpy(), want_s)
        assert (out_r[2] == -1).all()                                          # everything up to T is gone


# ---- 7. the eager form ----------------------------------------------------------------------------------------------------
def test_erase_remaps_the_tables_and_an_erased_memory_round_trips(tmp_path):
    from vidmem.memory import EmbeddingMemory, scope_of
    dtype, D = "bf16", 768
    cols = _columns("tagged_grouped", dtype, D)
    qbits = _data(dtype, D)[3]
    mem = _memory("tagged_grouped", CAP, D, dtype)
    kw = {"group": torch.from_numpy(np.array(cols.keys)), "tag": torch.from_numpy(np.array(cols.tags))}
    mem.append(from_bits(cols.rows, dtype), ids=[f"c_{i}" for i in range(N)], meta=[{"i": i} for i in range(N)], **kw)
    with pytest.raises(ValueError):
        mem.erase()
    with pytest.raises(ValueError):
        mem.erase(rows=[1], scope=scope_of(0))
    out = mem.erase(scope=[scope_of(1), scope_of(6, 0, 10 * MS)])             # 250 + 11 rows
    drop = E.mask_of_scopes(cols.tags, [scope_of(1), scope_of(6, 0, 10 * MS)])
    model = E.erase(cols, drop)
    assert out.count == 261 == model.count and len(mem) == N - 261 == len(mem.ids) == len(mem.meta)
    nro = out.new_row_of.cpu().numpy()
    assert np.array_equal(nro, model.new_row_of)
    for old in (0, 249, 500, 1511, N - 1):
        assert mem.id_of(int(nro[old])) == f"c_{old}" and mem.meta_of(int(nro[old])) == {"i": old}
    assert mem.id_of(len(mem)) is None
    out2 = mem.erase(rows=[0, 5])
    model2 = E.erase(model.cols, E.mask_of_rows(N - 261, [0, 5]))
    assert out2.count == 2 and mem.id_of(0) == "c_1" and mem.id_of(4) == "c_6"
    assert np.array_equal(E.compose(nro, out2.new_row_of.cpu().numpy()), E.compose(model.new_row_of, model2.new_row_of))
    path = str(tmp_path / "erased.npz")
    mem.snapshot(path)
    back = EmbeddingMemory.restore(path, capacity=CAP)
    assert back.tagged and back.grouped and len(back) == len(mem) and back.ids == mem.ids
    q = from_bits(qbits, dtype)
    for a, b in zip(mem.topk(q, 10) + mem.topk_grouped(q, 10) + mem.topk_scoped(q, 10, scope_of(3)),
                    back.topk(q, 10) + back.topk_grouped(q, 10) + back.topk_scoped(q, 10, scope_of(3))):
        assert torch.equal(a, b)
    _check_against_fresh(mem, "tagged_grouped", dtype, model2, N, qbits)
