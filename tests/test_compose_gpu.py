"""GPU: the look-ahead group search and row-sharded retrieval at 3 and 8 shards, and the three small kernels both are
built from - ``vm_cosine_exact``, ``vm_topk_select`` (with ``col_limit``), ``vm_topk_merge`` - against the host models of
tests/compose_ref.py (the C oracle, a stable argsort, a three-key sort).  tests/test_compose_cpu.py proves those models
and shows that the case tables used here tell the right rules from eight wrong ones.

Every comparison is bit for bit: row ids equal, scores equal as int64 views.  Nothing here has a tolerance, because
every value involved is the reference's fp64 arithmetic on the same 16-bit (or fp32) inputs.

  A  vm_cosine_exact     D down to 8 (16-bit) and 1 (fp32), S and Q around the 256-row block, zero / largest finite /
                         subnormal / one-element vectors, duplicates
  B  vm_topk_select      crafted fp64 matrices: ties across the per-thread stride and across col_limit, +-0.0, +-inf,
                         col_limit 0 / S / beyond S / negative / per query, k > S, row_base beyond 2**40
  C  vm_topk_merge       1, 2, 3, 8 parts: empty and ragged parts, ties within and across parts with the smaller row in
                         the later part, ids beyond 2**40, and one (score, row) in two parts (both copies come out)
  D  sharded retrieval   W = 3 and 8 shards in one process: (stride, offset) on the fast path, its redo and the
                         exhaustive route, shards with no row or fewer than k, rings, the emit cascade
  E  _group_search       the extractor's method on crafted embeddings against the chunk-by-chunk definition

With ``-s`` the module prints, per section, the most queries one fast-path call handed to the exhaustive redo.
"""
from __future__ import annotations

import ctypes as C
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import compose_ref as R
from tests import support
from tests import topk_plan as TP
from tests.support import TD

pytestmark = pytest.mark.gpu

APPENDS = (311, 1024, 97, 2048, 5)            # uneven append sizes, cycled
REDONE = {}                                   # section -> most queries one fast-path call redid exhaustively


def dev(bits: np.ndarray, dtype: str) -> torch.Tensor:
    """uint16 bit patterns (or float32 values, dtype 'f32') -> device tensor of that type, bits untouched."""
    a = np.ascontiguousarray(bits)
    if dtype == "f32":
        return torch.from_numpy(a.copy()).cuda()
    return torch.from_numpy(a.view(np.int16).copy()).cuda().view(TD[dtype])


def host(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def bit_equal(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64),
                                                 np.ascontiguousarray(b).view(np.int64))


def ctx():
    from vidmem import _lib
    return _lib.Context.get(0)


def ptr(t) -> C.c_void_p:
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def note_redone(section: str, n: int) -> None:
    REDONE[section] = max(REDONE.get(section, 0), int(n))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for section in sorted(REDONE):
        print(f"\n[compose] most queries redone exhaustively in one call, section {section}: {REDONE[section]}")


# ---------------------------------------------------------------------------------------------------------------------
# A. vm_cosine_exact
# ---------------------------------------------------------------------------------------------------------------------
def raw_cosine(q: torch.Tensor, r: torch.Tensor, S: int, D: int, dt: int):
    """One call of the C entry on a NaN-filled output (the memory's wrapper only reaches the memory's own D)."""
    from vidmem import _lib
    c = ctx()
    Q = q.shape[0]
    out = torch.full((Q, S), float("nan"), dtype=torch.float64, device="cuda")
    rc = c.L.vm_cosine_exact(c.handle, ptr(q), Q, ptr(r), S, D, dt, ptr(out), _lib.current_stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def check_cosine(out: np.ndarray, want: np.ndarray, Q: int, S: int, what):
    assert bit_equal(out, want[:Q, :S]), what
    if S > R.PLANT_ZERO:
        assert not out[:, R.PLANT_ZERO].any() and not np.signbit(out[:, R.PLANT_ZERO]).any(), what   # the norm guards
    assert not out[R.PLANT_ZERO].any(), what
    a, b, far = R.PLANT_DUP
    if S > b:       # an exact duplicate pair scores bitwise the same, also across the 256-row block edge
        assert bit_equal(out[:, a], out[:, b]), what
    if S > far:
        assert bit_equal(out[:, a], out[:, far]), what
    if Q > b:
        assert bit_equal(out[a], out[b]), what


@pytest.mark.parametrize("D", R.COS16_D)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_cosine_exact_16bit(dtype, D):
    from vidmem import _lib
    from vidmem.memory import EmbeddingMemory
    qb, rb = R.cosine_pair(dtype, D)
    want = R.oracle_matrix(qb, rb, dtype)
    assert np.isfinite(want).all()
    q, r = dev(qb, dtype), dev(rb, dtype)
    mem = EmbeddingMemory(8, D, dtype) if D == 128 else None
    for S, Q in itertools.product(R.COS_S, R.COS_Q):
        rc, out = raw_cosine(q[:Q].contiguous(), r[:S].contiguous(), S, D, _lib.DTYPES[dtype])
        assert rc == _lib.VM_OK, (S, Q, rc)
        check_cosine(out, want, Q, S, (dtype, D, S, Q))
        if mem is not None:     # the wrapper the extractor and the retrieval adapters call
            got = mem.cosine_exact(q[:Q], r[:S])
            assert got.dtype == torch.float64 and tuple(got.shape) == (Q, S)
            assert bit_equal(got.cpu().numpy(), want[:Q, :S]), (dtype, S, Q)
    if mem is not None:
        mem.close()


@pytest.mark.parametrize("D", R.COS32_D)
def test_cosine_exact_fp32(D):
    from vidmem.memory import EmbeddingMemory
    qb, rb = R.cosine_pair("f32", D)
    want = R.oracle_matrix(qb, rb, "f32")
    assert np.isfinite(want).all()
    q, r = dev(qb, "f32"), dev(rb, "f32")
    mem = EmbeddingMemory(8, 128, "f16")        # as_f32 scores the operands as they are, whatever the memory holds
    for S, Q in itertools.product(R.COS_S, R.COS_Q):
        got = mem.cosine_exact(q[:Q], r[:S], as_f32=True)
        assert got.dtype == torch.float64 and tuple(got.shape) == (Q, S)
        check_cosine(got.cpu().numpy(), want, Q, S, (D, S, Q))
    mem.close()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_cosine_exact_refuses_d_12_on_the_16bit_path(dtype):
    from vidmem import _lib
    x = torch.ones((4, 12), dtype=TD[dtype], device="cuda")
    rc, out = raw_cosine(x, x, 4, 12, _lib.DTYPES[dtype])
    assert rc == _lib.VM_ERR_UNSUPPORTED and np.isnan(out).all()


# ---------------------------------------------------------------------------------------------------------------------
# B. vm_topk_select
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", R.SEL_S)
def test_topk_select(S):
    from vidmem.memory import topk_select
    c = ctx()
    on_dev = {}
    n = 0
    for name, m, lim, k, base in R.select_cases((S,)):
        if id(m) not in on_dev:
            on_dev[id(m)] = torch.from_numpy(m).cuda()
        lim_t = None if lim is None else torch.from_numpy(lim).cuda()
        got = host(topk_select(c, on_dev[id(m)], k, col_limit=lim_t, row_base=base))
        want = R.select_ref(m, lim, k, base)
        assert R.same(got, want), (name, got[1][:3, :6], want[1][:3, :6])
        n += 1
    assert n == len(R.SEL_Q) * len(R.SEL_K) * len(R.SEL_LIMITS) * len(R.SEL_BASES)


def test_topk_select_keeps_the_bits_of_signed_zeros():
    """+0.0 and -0.0 tie, so the columns come out in column order, each with its own sign."""
    from vidmem.memory import topk_select
    m = np.array([[-0.0, 0.0, -1.0, -0.0, 0.0]])
    s, r = host(topk_select(ctx(), torch.from_numpy(m).cuda(), 5))
    assert r.tolist() == [[0, 1, 3, 4, 2]] and np.signbit(s).tolist() == [[True, False, True, False, True]]
    assert R.same((s, r), R.select_ref(m, None, 5))


# ---------------------------------------------------------------------------------------------------------------------
# C. vm_topk_merge
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", R.MRG_PARTS)
def test_topk_merge(parts):
    from vidmem.memory import topk_merge
    c = ctx()
    n = 0
    for k, Q in itertools.product(R.MRG_K, R.MRG_Q):
        s, r = R.merge_lists(parts, k, Q)
        got = host(topk_merge(c, torch.from_numpy(s).cuda(), torch.from_numpy(r).cuda()))
        want = R.merge_ref(s, r)
        assert R.same(got, want), (parts, k, Q, got[1][:3, :6], want[1][:3, :6])
        n += 1
    assert n == 12


def test_topk_merge_does_not_deduplicate():
    """One (score, row) in two parts: both copies come out, adjacent, the earlier part's first.  Callers merge disjoint
    row sets (include/vidmem.h); this pins what the kernel does with anything else."""
    from vidmem.memory import topk_merge
    c = ctx()
    s, r = R.merge_signed_zero_case()
    gs, gr = host(topk_merge(c, torch.from_numpy(s).cuda(), torch.from_numpy(r).cuda()))
    assert gr.tolist() == [[5, 5]] and np.signbit(gs).tolist() == [[False, True]]
    assert R.same((gs, gr), R.merge_ref(s, r))
    s, r = R.merge_query("shared", 3, 8, np.random.default_rng(1))
    gs, gr = host(topk_merge(c, torch.from_numpy(s[:, None]).cuda(), torch.from_numpy(r[:, None]).cuda()))
    assert R.same((gs, gr), R.merge_ref(s[:, None], r[:, None]))
    both = [int(x) for x in set(r[0]) & set(r[2]) if x >= 0]
    assert both and any(np.count_nonzero(gr[0] == x) == 2 for x in both)
    for x in both:                                     # wherever both copies made the list they sit side by side
        at = np.flatnonzero(gr[0] == x)
        assert at.size <= 2 and (at.size < 2 or at[1] == at[0] + 1)


# ---------------------------------------------------------------------------------------------------------------------
# D. sharded retrieval in one process
# ---------------------------------------------------------------------------------------------------------------------
def append_unevenly(mem, rows: torch.Tensor) -> None:
    lo, i = 0, 0
    while lo < rows.shape[0]:
        step = APPENDS[i % len(APPENDS)]
        mem.append(rows[lo:lo + step])
        lo, i = lo + step, i + 1


def build_shards(c: R.ShardCase, fill: bool = True):
    """W memories; shard g holds hist[g::W] (``fill=False``: nothing yet)."""
    from vidmem.memory import EmbeddingMemory
    shards = []
    for g in range(c.world):
        rows = c.hist[g::c.world]
        cap = c.cap or c.capacity or rows.shape[0] + 8
        mem = EmbeddingMemory(cap, c.D, c.dtype, ring=bool(c.cap))
        if fill and rows.shape[0]:
            append_unevenly(mem, dev(rows, c.dtype))
        shards.append(mem)
    return shards


def search_shards(shards, q: torch.Tensor, k: int, exact: bool, section: str, wrap=None):
    """Every shard's list with (stride, offset) = (W, g), and vm_topk_merge of the stack -> (merged, parts), host."""
    from vidmem.memory import topk_merge
    W = len(shards)
    S, Rr, rose = [], [], []
    for g, mem in enumerate(shards):
        mem.reset_uncertified()
        call = lambda: mem.topk(q, k, row_stride=W, row_offset=g, exact=exact)
        s, r = wrap(mem, call) if wrap else call()
        rose.append(mem.uncertified_count)
        S.append(s)
        Rr.append(r)
    note_redone(section, max(rose))
    S, Rr = torch.stack(S), torch.stack(Rr)
    return host(topk_merge(shards[0].ctx, S, Rr)), host((S, Rr)), rose


def check_sharded(c: R.ShardCase, shards, q, k, local, full, counts=None, section="D", wrap=None):
    """Default path and exact=True at one k: every part against the oracle of its own shard, the merge against the
    oracle over all live rows.  ``local`` / ``full``: the oracle's lists at the case's largest k."""
    want_parts = local[0][:, :, :k], R.shard_global(local[1][:, :, :k], c.hist.shape[0])
    want = full[0][:, :k], full[1][:, :k]
    rose = None
    for exact in ((False,) if k > 58 else (False, True)):     # k > 58: the default path IS the exhaustive route
        merged, parts, up = search_shards(shards, q, k, exact, section, wrap if not exact else None)
        rose = up if not exact else rose
        for g in range(c.world):
            assert R.same((parts[0][g], parts[1][g]), (want_parts[0][g], want_parts[1][g])), (c.name, k, exact, g, counts)
        assert R.same(merged, want), (c.name, k, exact, counts, merged[1][:3, :6], want[1][:3, :6])
    return rose, want


def close_all(shards):
    for mem in shards:
        mem.close()


@pytest.mark.parametrize("c", R.shard_cases(), ids=lambda c: c.name)
def test_sharded_retrieval(c):
    shards = build_shards(c)
    q = dev(c.queries, c.dtype)
    local = R.shard_local(c.queries, c.hist, R.SHARD_KMAX, c.dtype, c.world)
    full = R.sharded_ref(c.queries, c.hist, R.SHARD_KMAX, c.dtype, c.world)
    for k in c.ks:
        _, want = check_sharded(c, shards, q, k, local, full)
        for qi, ids in c.expect.items():      # the plants: duplicate pair, rotating run, zero query, stored row
            assert want[1][qi, :min(k, len(ids))].tolist() == ids[:k], (c.name, k, qi)
    close_all(shards)


def test_sharded_retrieval_redoes_an_uncertifiable_tie_on_every_shard():
    """tests/dist_worker.py's figures at W = 8: 20 identical rows on every shard and a query equal to them, k = 7.
    No shard's scan can certify that tie; each redoes the query before the merge (at least one counter must rise)."""
    c = R.dist_worker_case()
    shards = build_shards(c)
    k = c.ks[0]
    local = R.shard_local(c.queries, c.hist, k, c.dtype, c.world)
    full = R.sharded_ref(c.queries, c.hist, k, c.dtype, c.world)
    rose, want = check_sharded(c, shards, dev(c.queries, c.dtype), k, local, full, section="D dist-worker")
    assert max(rose) >= 1, rose
    for qi in (5, 15):
        assert want[1][qi].tolist() == list(range(1000, 1000 + k))       # the lowest ids, rotating through the shards
    close_all(shards)


def test_sharded_ring_shards_after_every_append():
    c = R.ring_case()
    shards = build_shards(c, fill=False)
    q = dev(c.queries, c.dtype)
    k = c.ks[0]
    per_shard = [dev(c.hist[g::c.world], c.dtype) for g in range(c.world)]
    have = [0] * c.world
    for counts in c.steps:
        for g, mem in enumerate(shards):
            mem.append(per_shard[g][have[g]:counts[g]])
        have = list(counts)
        assert [len(m) for m in shards] == have
        local = R.shard_local(c.queries, c.hist, k, c.dtype, c.world, counts, c.cap)
        full = R.sharded_ref(c.queries, c.hist, k, c.dtype, c.world, counts, c.cap)
        check_sharded(c, shards, q, k, local, full, counts=counts, section="D ring")
    assert have == [R.RING_FED] * c.world
    close_all(shards)


def test_sharded_retrieval_on_the_cascade():
    """The strided mapping on the emit cascade at stride 8: shards of capacity 65,536 (launches are sized from the
    capacity), and one call's scan / finalize launch counts are the plan's."""
    c = R.cascade_case()
    k, Q = R.CASCADE_K, R.CASCADE_Q
    plan = TP.plan(Q, k, c.D, c.dtype, R.CASCADE_CAP, torch.cuda.get_device_properties(0).multi_processor_count)
    assert plan.family == "cascade", plan
    shards = build_shards(c)
    assert all(m.capacity == R.CASCADE_CAP for m in shards)
    seen = []

    def counted(mem, call):
        out, launches = support.launches(mem, call)
        seen.append((launches["topk_scan"], launches["topk_finalize"]))
        return out

    local = R.shard_local(c.queries, c.hist, k, c.dtype, c.world)
    full = R.sharded_ref(c.queries, c.hist, k, c.dtype, c.world)
    check_sharded(c, shards, dev(c.queries, c.dtype), k, local, full, section="D cascade", wrap=counted)
    assert seen == [(plan.launches["topk_scan"], plan.launches["topk_finalize"])] * c.world, (seen, plan.launches)
    close_all(shards)


# ---------------------------------------------------------------------------------------------------------------------
# E. the extractor's look-ahead group search
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.group_cases(), ids=lambda c: c.name)
def test_group_search(c):
    from vidmem.extractor import FrameEmbeddingExtractor
    from vidmem.memory import EmbeddingMemory
    mem = EmbeddingMemory(c.capacity, c.D, c.dtype, ring=c.ring)
    if c.mem.shape[0]:
        mem.append(dev(c.mem, c.dtype))
    stand_in = SimpleNamespace(memory=mem, top_k=c.k)         # all the method uses of ``self``
    for j, (stored, emb) in enumerate(R.group_walk(c)):
        assert len(mem) == stored.shape[0] and len(mem) + emb.shape[0] <= mem.capacity    # the caller's guard
        emb_t = dev(emb, c.dtype)
        before = mem.uncertified_count
        got = host(FrameEmbeddingExtractor._group_search(stand_in, emb_t, list(c.counts)))
        note_redone("E", mem.uncertified_count - before)
        want = R.group_search_ref(stored, emb, c.counts, c.k, c.dtype)
        assert R.same(got, want), (c.name, j, c.contents[j], got[1][:4, :6], want[1][:4, :6])
        if not stored.shape[0]:      # the first chunk met an empty memory
            assert (got[1][:c.counts[0]] == -1).all() and not got[0][:c.counts[0]].any()
        mem.append(emb_t)
    if c.ring:
        assert len(mem) == mem.capacity          # filled exactly, nothing overwritten
    mem.close()
