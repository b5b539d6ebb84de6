"""GPU: group summaries (vm_memory_summaries, csrc/summary.hip) against tests/summary_ref.py.

Bar: bit equality of every output - first rows, row counts, keys, centroid bits, key rows, key scores as int64 views,
the padding and the count - on sentinel-filled buffers a few entries longer than needed, with the sentinels behind them
untouched.  The data sets and their oracle summaries are made once and shared.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import events_ref as E
from tests import summary_ref as S
from tests.search_checks import RING_CAP, ptr, raw_regroup
from tests.support import from_bits, same_bits

pytestmark = pytest.mark.gpu

SENT_I, SENT_S, SENT_C = -7, 123.0, 0x5555          # what the output buffers hold before a call
ROOM = 3


def grouped_memory(bits, keys, dtype, capacity=None, ring=False, tags=None, step=1000):
    """A grouped memory appended ``bits`` with ``keys`` (None: plain appends, every row its own group)."""
    from vidmem.memory import EmbeddingMemory
    n = bits.shape[0]
    mem = EmbeddingMemory(capacity or max(n, 1), bits.shape[1], dtype, ring=ring, grouped=True, tagged=tags is not None)
    step = min(step, mem.capacity)
    for c0 in range(0, n, step):
        rows = from_bits(bits[c0:c0 + step], dtype)
        if keys is None:
            first = C.c_int64(0)
            from vidmem import _lib
            mem.ctx.check(mem.L.vm_memory_append(mem.handle, ptr(rows), rows.shape[0], C.byref(first),
                                                 _lib.current_stream_ptr()))
            mem.ids.extend([None] * rows.shape[0])
            mem.meta.extend([None] * rows.shape[0])
        else:
            mem.append(rows, group=torch.from_numpy(np.ascontiguousarray(keys[c0:c0 + step])),
                       tag=None if tags is None else torch.from_numpy(np.ascontiguousarray(tags[c0:c0 + step])))
        torch.cuda.synchronize()
    mem.sync()
    return mem


def ws_need(mem, max_groups):
    need = int(mem.L.vm_memory_summaries_workspace_bytes(mem.handle, int(max_groups)))
    m = min(max_groups, mem.capacity)
    assert 0 < need <= 8 * (mem.capacity + 256) + m * (2 * mem.dim + 8) + 2048, need
    return need


class Raw:
    """One call of the C entry on sentinel-filled buffers ROOM entries longer than ``max_groups``; the whole buffers as
    numpy arrays (``None`` for an output passed as NULL)."""

    def __init__(self, mem, first_group=None, max_groups=0, skip=(), ws_bytes=None):
        from vidmem import _lib
        need = ws_need(mem, max_groups)
        ws = torch.empty(max(need if ws_bytes is None else ws_bytes, 256), dtype=torch.uint8, device="cuda")
        m = max_groups + ROOM
        buf = {"centroids": torch.full((m, mem.dim), SENT_C, dtype=torch.int16, device="cuda"),
               "first_rows": torch.full((m,), SENT_I, dtype=torch.int64, device="cuda"),
               "n_rows": torch.full((m,), SENT_I, dtype=torch.int64, device="cuda"),
               "keys": torch.full((m,), SENT_I, dtype=torch.int64, device="cuda"),
               "key_rows": torch.full((m,), SENT_I, dtype=torch.int64, device="cuda"),
               "key_scores": torch.full((m,), SENT_S, dtype=torch.float64, device="cuda")}
        cnt = torch.full((1,), SENT_I, dtype=torch.int64, device="cuda")
        frm = None
        if first_group is not None:
            frm = first_group if isinstance(first_group, torch.Tensor) else \
                torch.tensor([int(first_group)], dtype=torch.int64).cuda()
        arg = lambda name: ptr(None if name in skip else buf[name])
        self.rc = mem.L.vm_memory_summaries(mem.handle, ptr(frm), int(max_groups), arg("centroids"), arg("first_rows"),
                                            arg("n_rows"), arg("keys"), arg("key_rows"), arg("key_scores"), ptr(cnt),
                                            ptr(ws), need if ws_bytes is None else ws_bytes, _lib.current_stream_ptr())
        torch.cuda.synchronize()
        self.count = int(cnt.item())
        self.max_groups = max_groups
        for name, t in buf.items():
            a = t.cpu().numpy()
            setattr(self, name, a.view(np.uint16) if name == "centroids" else a)

    def untouched(self, names=None, start=None):
        """The entries from ``start`` on (default: behind max_groups) still hold the sentinels."""
        at = self.max_groups if start is None else start
        every = ("centroids", "first_rows", "n_rows", "keys", "key_rows", "key_scores")
        for name in every if names is None else names:
            a = getattr(self, name)[at:]
            sent = SENT_C if name == "centroids" else SENT_S if name == "key_scores" else SENT_I
            if not (a == sent).all():
                return False
        return True


def check(mem, want: S.Summary, first_group=None, max_groups=None, skip=(), label=""):
    """vm_memory_summaries of ``mem`` through one window against the oracle's summary of ALL its live groups."""
    G = want.first_rows.size
    mg = G + 2 if max_groups is None else max_groups
    got = Raw(mem, first_group, mg, skip)
    assert got.rc == 0, (label, got.rc, mem.L.vm_last_error(mem.ctx.handle))
    assert got.count == G, (label, got.count, G)
    w = S.window(want, 0 if first_group is None else first_group, mg, mem.dim)
    for name in ("first_rows", "n_rows", "keys", "key_rows"):
        if name not in skip:
            a, b = getattr(got, name)[:mg], getattr(w, name)
            assert np.array_equal(a, b), (label, name, np.argwhere(a != b)[:5].ravel(), a[a != b][:5], b[a != b][:5])
    if "centroids" not in skip:
        bad = np.argwhere(got.centroids[:mg] != w.centroids)
        assert bad.size == 0, (label, "centroid bits", bad[:5].tolist())
    if "key_scores" not in skip:
        assert same_bits(got.key_scores[:mg], w.key_scores), \
            (label, "key scores (bit-exact bar)", np.argwhere(got.key_scores[:mg] != w.key_scores)[:5].ravel())
    assert got.untouched(), (label, "sentinels behind max_groups")
    assert got.untouched(skip, start=0), (label, "an output passed as NULL")
    return got


@functools.lru_cache(maxsize=None)
def scene_keys(name):
    sizes = E.dataset(name)[2]
    return np.repeat(np.arange(len(sizes), dtype=np.int64) + 1000, sizes)


@functools.lru_cache(maxsize=None)
def scene_summary(name, lo=0):
    """The oracle summary of rows lo .. of a planted-scene set with one key per scene: made once, never modified."""
    dtype, bits, _, _ = E.dataset(name)
    return S.summarize(bits[lo:], scene_keys(name)[lo:], dtype, base=lo)


# ---- 1. planted scenes as chunks: linear and wrapped ---------------------------------------------------------------------
@pytest.mark.parametrize("ring", [False, True], ids=["linear", "ring"])
@pytest.mark.parametrize("name", list(E.SETS))
def test_planted_scenes(name, ring):
    dtype, bits, sizes, _ = E.dataset(name)
    n = bits.shape[0]
    cap = RING_CAP[name] if ring else None
    lo = n - cap if ring else 0
    keys = scene_keys(name)
    mem = grouped_memory(bits, keys, dtype, capacity=cap, ring=ring)
    if ring:        # the oldest group is partial, and a group straddles the physical wrap (row id = capacity)
        assert keys[lo] == keys[lo - 1] and keys[cap] == keys[cap - 1] and lo < cap < n
    want = scene_summary(name, lo)
    G = want.first_rows.size
    assert G == len(sizes) - (keys[lo] - 1000) and want.n_rows.max() <= 23 and want.n_rows.min() == 1
    check(mem, want, label=f"{name} ring={ring}")
    # the Python entry: trimmed, the full count
    got = mem.summaries()
    assert got.count == G and np.array_equal(got.first_rows.cpu().numpy(), want.first_rows)
    assert np.array_equal(got.centroids.view(torch.int16).cpu().numpy().view(np.uint16), want.centroids)
    assert np.array_equal(got.key_rows.cpu().numpy(), want.key_rows)
    assert same_bits(got.key_scores.cpu().numpy(), want.key_scores)
    cut = mem.summaries(first_group=3, max_groups=4)
    assert cut.count == G and cut.keys.tolist() == want.keys[3:7].tolist() and cut.n_rows.tolist() == want.n_rows[3:7].tolist()


# ---- 2. windows ------------------------------------------------------------------------------------------------------------
def test_windows():
    name = "f16_128"
    dtype, bits, _, _ = E.dataset(name)
    mem = grouped_memory(bits, scene_keys(name), dtype)
    want = scene_summary(name)
    G = want.first_rows.size
    dev = torch.tensor([G // 2], dtype=torch.int64, device="cuda")
    for g0, mg in ((0, 1), (0, 5), (G // 2, 7), (dev, 7), (G - 1, 1), (G - 1, 4), (G - 3, G + 5), (-4, 3), (None, G),
                   (0, G + 9)):
        first = g0 if not isinstance(g0, torch.Tensor) else G // 2
        check(mem, want, first if isinstance(g0, torch.Tensor) else g0, mg, label=f"window {first} {mg}")
        if isinstance(g0, torch.Tensor):
            got = Raw(mem, g0, mg)
            assert np.array_equal(got.first_rows[:mg], S.window(want, G // 2, mg, 128).first_rows)
    # first_group >= n_groups: the count and the padding
    for g0 in (G, G + 100):
        got = check(mem, want, g0, 4, label="beyond the last group")
        assert (got.first_rows[:4] == -1).all() and (got.key_scores[:4] == 0.0).all() and not got.centroids[:4].any()
    # max_groups = 0: the count only, the other outputs may be NULL
    got = Raw(mem, 0, 0, skip=("centroids", "first_rows", "n_rows", "keys", "key_rows", "key_scores"))
    assert got.rc == 0 and got.count == G and got.untouched(start=0)
    got = Raw(mem, 5, 0)
    assert got.rc == 0 and got.count == G and got.untouched(start=0)
    # one group asked through two windows: the same bits
    a, b = Raw(mem, 10, 20), Raw(mem, 17, 3)
    for name_ in ("centroids", "first_rows", "n_rows", "keys", "key_rows"):
        assert np.array_equal(getattr(a, name_)[7:10], getattr(b, name_)[:3])
    assert same_bits(a.key_scores[7:10], b.key_scores[:3])
    # key outputs NULL: the same centroids; each output may be NULL on its own
    check(mem, want, 3, 50, skip=("key_rows", "key_scores"), label="no key frames")
    check(mem, want, 3, 50, skip=("key_rows",), label="scores without rows")
    check(mem, want, 3, 50, skip=("centroids",), label="no centroids")
    check(mem, want, 3, 50, skip=("centroids", "key_rows", "key_scores", "keys"), label="bounds only")
    check(mem, want, 3, 50, skip=("first_rows", "n_rows"), label="no bounds")


# ---- 3. events as groups, and an erase that joins two groups ------------------------------------------------------------
def test_after_regroup_events_and_after_erase():
    name = "f16_768"
    dtype, bits_ro, sizes, link_all = E.dataset(name)
    n = 1500
    bits = bits_ro[:n]
    mem = grouped_memory(bits, np.arange(n, dtype=np.int64) // 16, dtype)           # fixed chunks of 16 first
    check(mem, S.summarize(bits, np.arange(n) // 16, dtype), label="chunks of 16")
    flags = E.opens(link_all[:n], 0.5)
    want_re = E.regroup(flags)
    assert raw_regroup(mem, 0.5) == (0, want_re.state[0])
    check(mem, S.summarize(bits, want_re.keys, dtype), label="groups = events")
    # two groups with one key become adjacent: ONE group afterwards
    keys = np.repeat(np.array([5, 6, 5, 7], np.int64), [10, 4, 9, 6])
    small = bits_ro[:29]
    mem2 = grouped_memory(small, keys, dtype)
    check(mem2, S.summarize(small, keys, dtype), label="before the erase")
    assert mem2.erase(rows=list(range(10, 14))).count == 4
    mem2.sync()
    keep = np.ones(29, bool)
    keep[10:14] = False
    want = S.summarize(np.ascontiguousarray(small[keep]), keys[keep], dtype)
    assert want.n_rows.tolist() == [19, 6]
    check(mem2, want, label="after an erase that joins two groups")


# ---- 4. plain appends: every row its own group ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bf16_1024", "f16_128"])
def test_plain_appended_rows_are_their_own_groups(name):
    dtype, bits_ro, _, _ = E.dataset(name)
    n = 300
    bits = bits_ro[:n]
    mem = grouped_memory(bits, None, dtype)
    want = S.summarize(bits, -1 - np.arange(n, dtype=np.int64), dtype)
    assert want.n_rows.tolist() == [1] * n and np.array_equal(want.key_rows, np.arange(n))
    check(mem, want, label="plain appends")


# ---- 5. special groups -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_special_groups(dtype):
    groups = S.special_groups(dtype)
    bits = np.ascontiguousarray(np.vstack([g for _, g in groups]))
    keys = np.repeat(np.arange(len(groups), dtype=np.int64), [g.shape[0] for _, g in groups])
    want = S.summarize(bits, keys, dtype)
    names = [nm for nm, _ in groups]
    z, c, i, s = (names.index(x) for x in ("zeros", "cancel", "identical", "subnormal"))
    for g in (z, c):        # all-zero rows; {x, -x} cancels exactly: the zero centroid, score 0.0, the first row
        assert not want.centroids[g].any() and want.key_scores[g] == 0.0 and want.key_rows[g] == want.first_rows[g]
    assert want.key_rows[i] == want.first_rows[i] and want.n_rows[i] == 5           # identical rows: the lowest id
    assert want.centroids[s].any()
    if dtype == "bf16":
        o = names.index("order")
        assert (want.centroids[o] != S.centroid(groups[o][1], dtype, reverse=True)).any()
    mem = grouped_memory(bits, keys, dtype, capacity=64)
    check(mem, want, label=f"special groups {dtype}")


# ---- 6. long groups ------------------------------------------------------------------------------------------------------------
def _long_rows(n, dtype, seed):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(128)
    return S.f64_to_bits(base[None, :] * 0.5 + rng.standard_normal((n, 128)), dtype)


@pytest.mark.parametrize("dtype,n", [("bf16", 3000), ("f16", 9000)])
def test_one_long_group(dtype, n):
    """One group of 3,000 bf16 rows / 9,000 fp16 rows (above the 2^13 rows up to which an fp16 sum is exact in any
    order), with a short group before and after it."""
    bits = _long_rows(n + 9, dtype, 21)
    keys = np.repeat(np.array([1, 2, 3], np.int64), [4, n, 5])
    mem = grouped_memory(bits, keys, dtype, step=4096)
    want = S.summarize(bits, keys, dtype)
    assert want.n_rows.tolist() == [4, n, 5]
    check(mem, want, label=f"long group {dtype}")
    check(mem, want, 1, 1, label="the long group alone")


def test_four_thousand_groups_of_one_row():
    bits = _long_rows(4000, "f16", 22)
    keys = np.arange(4000, dtype=np.int64) * 3
    mem = grouped_memory(bits, keys, "f16", step=4096)
    want = S.summarize(bits, keys, "f16")
    assert np.array_equal(want.key_rows, np.arange(4000))
    check(mem, want, label="4,000 groups of one row")
    check(mem, want, 1234, 1000, label="a window of them")


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    from vidmem import _lib
    from vidmem.memory import EmbeddingMemory
    from tests.search_checks import raw_append_memory
    dtype, bits, _, _ = E.dataset("f16_128")
    plain = raw_append_memory(bits[:64], dtype)                          # not grouped
    got = Raw(plain, 0, 8)
    assert got.rc == _lib.VM_ERR_INVALID and got.count == SENT_I and got.untouched(start=0)
    with pytest.raises(ValueError, match="grouped"):
        plain.summaries()
    mem = grouped_memory(bits[:777], scene_keys("f16_128")[:777], dtype)
    need = ws_need(mem, 8)
    got = Raw(mem, 0, 8, ws_bytes=need - 1)                   # a short workspace: refused before any launch
    assert got.rc == _lib.VM_ERR_NOMEM and got.count == SENT_I and got.untouched(start=0)
    outs = [Raw(mem, 2, 8, ws_bytes=b) for b in (need, need + 256, need + 12345)]      # the size does not matter
    for other in outs[1:]:
        assert other.rc == 0 and other.count == outs[0].count
        assert np.array_equal(other.centroids, outs[0].centroids) and same_bits(other.key_scores, outs[0].key_scores)
        assert np.array_equal(other.key_rows, outs[0].key_rows)
    got = Raw(mem, 0, -1)
    assert got.rc == _lib.VM_ERR_INVALID and got.count == SENT_I
    empty = EmbeddingMemory(32, 128, dtype, grouped=True)     # an empty memory: the count and nothing else
    got = Raw(empty, 0, 8)
    assert got.rc == 0 and got.count == 0 and got.untouched(start=0)
    s = empty.summaries()
    assert s.count == 0 and s.first_rows.numel() == 0 and s.centroids.shape == (0, 128)


# ---- 8. graph capture ----------------------------------------------------------------------------------------------------------
def test_graph_capture_append_and_summaries_replayed():
    from vidmem.memory import EmbeddingMemory
    name = "f16_768"
    dtype, bits_ro, _, _ = E.dataset(name)
    keys_all = scene_keys(name)
    B, H = 128, 64
    mem = EmbeddingMemory(1024, 768, dtype, grouped=True)
    mem.append(from_bits(bits_ro[:256], dtype), group=torch.from_numpy(keys_all[:256]))
    scratch = mem.prepare_summaries(H)
    src = from_bits(bits_ro[256:256 + B], dtype).clone()
    src_keys = torch.from_numpy(keys_all[256:256 + B]).cuda()
    frm = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            mem.append(src, group=src_keys)
            out = mem.enqueue_summaries(frm, max_groups=H, scratch=scratch)
    torch.cuda.current_stream().wait_stream(s)
    mem.sync()                     # the capture advanced only the host mirror: back to the device count
    assert len(mem) == 256
    for rep in range(3):
        n = 256 + (rep + 1) * B
        src.copy_(from_bits(bits_ro[n - B:n], dtype))
        src_keys.copy_(torch.from_numpy(keys_all[n - B:n]))
        frm.fill_(rep * 5)         # the window pages between replays
        graph.replay()
        torch.cuda.synchronize()
        assert mem.sync() == n
        want = S.summarize(bits_ro[:n], keys_all[:n], dtype)
        w = S.window(want, rep * 5, H, 768)
        assert int(out.count.item()) == want.first_rows.size
        assert np.array_equal(out.first_rows.cpu().numpy(), w.first_rows)
        assert np.array_equal(out.n_rows.cpu().numpy(), w.n_rows) and np.array_equal(out.keys.cpu().numpy(), w.keys)
        assert np.array_equal(out.centroids.view(torch.int16).cpu().numpy().view(np.uint16), w.centroids)
        assert np.array_equal(out.key_rows.cpu().numpy(), w.key_rows)
        assert same_bits(out.key_scores.cpu().numpy(), w.key_scores)
