"""Test support: what more than one test file needs to build data, memories and operands, and the one checker of the
searches that have a fast and an ``exact=True`` entry (``check_entries``, ``redone``, ``scan_memory``).  A plain module,
not a conftest: no fixtures, imported by name.  It imports without a GPU; whatever touches the device does so inside a
function.  The data of the tile-scan shapes is in tests/tile_scan_data.py, the checkers of single searches that a second
file uses in tests/search_checks.py.
"""
import numpy as np
import torch

TD = {"f16": torch.float16, "bf16": torch.bfloat16}
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
ALL = (INT64_MIN, INT64_MAX)        # the scope that holds every tag
MS = 33                             # milliseconds between the rows of one source


# ---- bit patterns -----------------------------------------------------------------------------------------------------
def bits(t: torch.Tensor) -> np.ndarray:
    """uint16 bit patterns of a 16-bit torch tensor (host copy)."""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def from_bits(b, dtype="f16") -> torch.Tensor:
    """uint16 bit patterns -> device tensor of the memory dtype."""
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int16)).view(TD[dtype]).cuda()


def to_bits(x, dtype) -> np.ndarray:
    """fp32 values (fp64 is rounded to fp32 first) -> the uint16 bit patterns of their round-to-nearest-even f16 / bf16
    images, as torch rounds.  No NaN / inf in these tests.  tests/test_support_cpu.py holds it against the rounding done
    by hand on every 16-bit pattern and around every midpoint."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(TD[dtype])
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def np_of(x) -> np.ndarray:
    """A device tensor, a host tensor or an array -> numpy."""
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


# ---- data -------------------------------------------------------------------------------------------------------------
def group_sizes(n_groups, size, seed):
    if size == "ragged":
        rng = np.random.default_rng(seed)
        return [int(x) for x in rng.integers(1, 24, n_groups)]
    return [size] * n_groups


def clustered(sizes, D, dtype, seed, noise=0.05, device="cuda"):
    """Rows of len(sizes) groups; group g = a random centre + small per-row noise (one scene, consecutive frames)."""
    g = torch.Generator(device=device).manual_seed(seed)
    n = int(sum(sizes))
    centres = torch.randn(len(sizes), D, generator=g, device=device)
    gid = torch.repeat_interleave(torch.arange(len(sizes), device=device), torch.tensor(sizes, device=device))
    rows = centres[gid] + noise * torch.randn(n, D, generator=g, device=device)
    rows = rows / rows.norm(dim=1, keepdim=True)
    return rows.to(TD[dtype]), gid


def queries_near(rows, Q, seed, dtype):
    g = torch.Generator(device=rows.device).manual_seed(seed)
    pick = torch.randint(0, rows.shape[0], (Q,), generator=g, device=rows.device)
    q = rows[pick].float() + 0.1 * torch.randn(Q, rows.shape[1], generator=g, device=rows.device)
    return q.to(TD[dtype])


def planted_duplicates(n_dup_step=24):
    """3,000 random rows with 40 copies of row 5 among rows 1,010 .. 1,969 -> (rows, the planted row, the copies' ids)."""
    rows = torch.randn(3000, 768, device="cuda", generator=torch.Generator("cuda").manual_seed(2)).to(torch.float16)
    row = rows[5].clone()
    dup = list(range(1010, 1970, n_dup_step))          # 40 copies: k = 10 keeps 18 candidates
    for r in dup:
        rows[r] = row
    return rows, row, dup


# ---- tags -------------------------------------------------------------------------------------------------------------
def make_tag(source, ms):
    return (int(source) << 40) | int(ms)


def scope_of(source, t0=None, t1=None):
    return make_tag(source, 0 if t0 is None else t0), make_tag(source, (1 << 40) - 1 if t1 is None else t1)


def contiguous_tags(n, sources):
    """n rows in `sources` contiguous videos of n / sources rows, MS apart."""
    per = n // sources
    i = np.arange(n, dtype=np.int64)
    return ((i // per) << 40) | ((i % per) * MS)


def mixed_scopes(tags, Q, k):
    """At least 5 distinct scopes in one call: no row at all, lo > hi, one row, fewer than k rows, a sub-window of a
    video, a whole video, everything."""
    one = int(tags[len(tags) // 3])
    pool = [scope_of(100), (10, 5), (one, one), scope_of(5, 0, MS * max(k - 2, 0)), scope_of(3, MS * 100, MS * 300),
            scope_of(6), ALL]
    return [pool[i % len(pool)] for i in range(Q)]


# ---- memories ---------------------------------------------------------------------------------------------------------
def plain_memory(rows, dtype, capacity=None, ring=False, step=65536, **kind):
    from vidmem.memory import EmbeddingMemory
    mem = EmbeddingMemory(capacity or max(rows.shape[0], 16), rows.shape[1], dtype, ring=ring, **kind)
    step = min(step, mem.capacity)
    for c0 in range(0, rows.shape[0], step):
        mem.append(rows[c0:c0 + step])
    return mem


def grouped_memory(rows, sizes, dtype, capacity=None, ring=False, keys=None):
    from vidmem.memory import EmbeddingMemory
    mem = EmbeddingMemory(capacity or max(rows.shape[0], 16), rows.shape[1], dtype, ring=ring, grouped=True)
    off = 0
    for i, s in enumerate(sizes):
        mem.append(rows[off:off + s], group=None if keys is None else keys[i])
        off += s
    return mem


def tagged_memory(rows, tags, dtype, capacity=None, ring=False, step=65536, **kind):
    from vidmem.memory import EmbeddingMemory
    mem = EmbeddingMemory(capacity or max(rows.shape[0], 16), rows.shape[1], dtype, ring=ring, tagged=True, **kind)
    tags = torch.as_tensor(np.asarray(tags, dtype=np.int64), device=rows.device)
    step = min(step, mem.capacity)
    for c0 in range(0, rows.shape[0], step):
        mem.append(rows[c0:c0 + step], tag=tags[c0:c0 + step])
    return mem


# ---- operands ---------------------------------------------------------------------------------------------------------
def dev_mask(words) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).cuda()


def dev_bias(cols) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(cols, dtype=np.float32)).cuda()


class Embedder:
    """A text embedder that answers every query with one vector."""

    def __init__(self, vec):
        self.vec = vec

    async def aembed_query(self, text):
        return self.vec


# ---- comparisons ------------------------------------------------------------------------------------------------------
def same_result(a, b) -> bool:
    """Two (scores, rows) pairs of tensors, as a search returns them: rows equal, scores equal bit for bit."""
    return torch.equal(a[1], b[1]) and np.array_equal(a[0].cpu().numpy().view(np.int64), b[0].cpu().numpy().view(np.int64))


def same_bits(a, b) -> bool:
    """Two arrays of fp64 values equal bit for bit."""
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


def same_arrays(a, b) -> bool:
    """Two (rows, scores) pairs of arrays, as an oracle returns them: rows equal, scores equal bit for bit.  Whatever
    follows the pair is not looked at."""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int64), b[1].view(np.int64))


def launches(mem, fn, counters=("topk_scan", "topk_finalize", "topk_exact")):
    """fn() with the context's launch counters on -> (what fn returned, {counter: launches})."""
    ctx = mem.ctx
    ctx.profile_mask(None)
    ctx.profile_enable(256)
    try:
        out = fn()
        prof = ctx.profile_read()
    finally:
        ctx.profile_enable(0)
    return out, {c: prof[c][1] for c in counters}


# ---- the checker of the searches with a fast and an exact entry -------------------------------------------------------
def _differences(got, want, limit=5):
    """The first few positions at which two equal-shaped arrays differ, with both values (fp64: with their bits too)."""
    as_bits = want.dtype == np.float64
    g, w = (got.view(np.int64), want.view(np.int64)) if as_bits else (got, want)
    out = []
    for at in np.argwhere(g != w)[:limit]:
        at = tuple(int(i) for i in at)
        if as_bits:
            out.append(f"{list(at)}: got {float(got[at])!r} ({int(g[at]) & (2 ** 64 - 1):#018x}), "
                       f"want {float(want[at])!r} ({int(w[at]) & (2 ** 64 - 1):#018x})")
        else:
            out.append(f"{list(at)}: got {got[at]}, want {want[at]}")
    return f"{int((g != w).sum())} differ; " + "; ".join(out)


def check_entries(call, flags_of, want, certified=None, label=""):
    """The fast and the exact entry of one search against ``want``.

    call(exact)  runs the search and returns its outputs, arrays or tensors, in the order of ``want``.
    flags_of()   the fast entry's per-query flags; read right after the fast call.
    want         a tuple of arrays: rows first, then scores, then whatever else the search returns.
    certified    None, True, or a bool per query: the fast entry must have answered those queries itself (flag 0).

    For both entries every output equals its ``want`` in shape, in dtype and in content: fp64 outputs as int64 bit
    patterns (+0.0 is not -0.0), integer outputs by value, the -1 / 0.0 padding included.
    -> (*outputs of the fast entry, flags)."""
    out = None
    for exact in (False, True):
        entry = "exact" if exact else "fast"
        got = tuple(np_of(x) for x in call(exact))
        if not exact:
            flags = np_of(flags_of())
            out = (*got, flags)
        assert len(got) == len(want), f"{label}: the {entry} entry returned {len(got)} outputs, want {len(want)}"
        for i, (g, w) in enumerate(zip(got, want)):
            what = f"{label}: {('rows', 'scores')[i] if i < 2 else f'output {i}'} of the {entry} entry"
            assert g.shape == w.shape, f"{what}: shape {g.shape}, want {w.shape}"
            assert g.dtype == w.dtype, f"{what}: dtype {g.dtype}, want {w.dtype}"
            same = np.array_equal(g.view(np.int64), w.view(np.int64)) if w.dtype == np.float64 else np.array_equal(g, w)
            assert same, f"{what} differ{' (bit-exact bar)' if w.dtype == np.float64 else ''}: {_differences(g, w)}"
        if not exact and certified is not None and certified is not False:
            demanded = flags if certified is True else flags[np.asarray(certified, dtype=bool)]
            assert (demanded == 0).all(), f"{label}: the scan left queries to the redo: {flags}"
    return out


def redone(check, count, Q, label="", flag=None):
    """A call that the fast path must hand to the exhaustive redo.  check() runs a search's checker -> (rows, scores, ...,
    flags); count() reads the search's uncertified counter.  Every flag is set - to ``flag`` when one is given -, the
    first is GAP or OVERFLOW, and the counter went up by Q.  -> (rows, scores)."""
    from vidmem import _lib
    before = count()
    got = check()
    flags = got[-1]
    assert (flags != 0).all(), f"{label}: a query was not left to the redo: {flags}"
    if flag is not None:
        assert (flags == flag).all(), f"{label}: flags {flags}, want {flag} for every query"
    assert flags[0] in (_lib.VM_FLAG_GAP, _lib.VM_FLAG_OVERFLOW), f"{label}: flag {flags[0]} is neither GAP nor OVERFLOW"
    after = count()
    assert after == before + Q, f"{label}: the uncertified counter went from {before} to {after}, want + {Q}"
    return got[0], got[1]


def scan_memory(D, dtype, shape):
    """What every scan test begins with: the tile-scan data set of ``shape`` on the device, held against the host's
    bit for bit, in a memory appended 19 rows at a time (a ring where the shape has a capacity).
    -> (mem, q_all, base, live, total, cap)."""
    from tests import mask_ref as MR
    from tests.tile_scan_data import dataset
    rows, q_all, base, live = dataset(D, dtype, shape)
    hrows, hq, hbase, hlive = MR.host_dataset(D, dtype, shape)
    assert hbase == base and np.array_equal(bits(rows), bits(hrows)) and np.array_equal(bits(q_all), bits(hq)), \
        f"{shape} D={D} {dtype}: the device data set is not its host twin"
    total, cap = MR.SHAPES[shape]
    mem = plain_memory(rows, dtype, capacity=cap, ring=cap is not None, step=19)
    assert mem.rows_host()[0] == base, f"{shape} D={D} {dtype}: base {mem.rows_host()[0]}, want {base}"
    return mem, q_all, base, live, total, cap
