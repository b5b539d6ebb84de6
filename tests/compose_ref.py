"""Host models and case tables of the two COMPOSED searches: the look-ahead group search of the extractor
(``memory.topk`` + ``vm_cosine_exact`` + ``vm_topk_select`` + ``vm_topk_merge``) and row-sharded retrieval
(``topk(row_stride=W, row_offset=g)`` per shard + ``vm_topk_merge`` of W lists).  numpy and the C oracle only.

tests/test_compose_cpu.py proves the models against each other and shows that every case table tells the right
rules from eight wrong ones; tests/test_compose_gpu.py runs the same tables through the kernels.  Everything here is
the reference's fp64 arithmetic, so every comparison built on it is bit for bit.
"""
from __future__ import annotations

import itertools
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from oracle import cref
from tests.support import to_bits

# ---------------------------------------------------------------------------------------------------------------------
# bit patterns
# ---------------------------------------------------------------------------------------------------------------------
THREADS = min(8, os.cpu_count() or 1)                  # the oracle's thread pool
MAX_FINITE = {"f16": 0x7BFF, "bf16": 0x7F7F}          # 65504, 3.3895e38
SUBNORMAL_MASK = {"f16": 0x03FF, "bf16": 0x007F}      # exponent field 0, any mantissa


def unit_bits(rng: np.random.Generator, n: int, D: int, dtype: str) -> np.ndarray:
    """n random unit rows as 16-bit patterns."""
    x = rng.standard_normal((n, D)).astype(np.float32)
    x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-6)
    return to_bits(x, dtype)


def same(a: Tuple[np.ndarray, np.ndarray], b: Tuple[np.ndarray, np.ndarray]) -> bool:
    """(scores, rows) pairs equal bit for bit: row ids equal, scores equal as int64 views (+0.0 != -0.0 here)."""
    return (a[0].shape == b[0].shape and np.array_equal(a[1], b[1])
            and np.array_equal(np.ascontiguousarray(a[0]).view(np.int64), np.ascontiguousarray(b[0]).view(np.int64)))


def _padded(Q: int, k: int):
    return np.zeros((Q, k), np.float64), np.full((Q, k), -1, np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# the models.  Every one returns (scores [Q,k] fp64, rows [Q,k] int64), the order of the library's own results.
# ---------------------------------------------------------------------------------------------------------------------
def select_ref(scores: np.ndarray, col_limit, k: int, row_base: int = 0, *, inclusive: bool = False,
               ties_descending: bool = False, ignore_limit: bool = False):
    """vm_topk_select: per query a stable argsort of -scores[q, :clamp(col_limit[q], 0, S)], the first k kept, -1 / 0.0
    padded; ``col_limit=None`` means S; rows = row_base + column.  The keyword switches are the planted defects of
    tests/test_compose_cpu.py (``<= col_limit``, ties by column descending, no limit at all)."""
    Q, S = scores.shape
    out_s, out_r = _padded(Q, k)
    for q in range(Q):
        n = S
        if col_limit is not None and not ignore_limit:
            n = min(max(int(col_limit[q]) + (1 if inclusive else 0), 0), S)
        row = scores[q, :n]
        if ties_descending:
            order = (n - 1 - np.argsort(-row[::-1], kind="stable"))[:k]
        else:
            order = np.argsort(-row, kind="stable")[:k]
        out_s[q, :order.size] = row[order]
        out_r[q, :order.size] = row_base + order
    return out_s, out_r


def merge_ref(scores: np.ndarray, rows: np.ndarray, *, ties_by_part: bool = False, drop_equal: bool = False):
    """vm_topk_merge of [parts,Q,k] lists: entries with row < 0 dropped; order = score descending, then row ascending,
    then position in the part-major concatenation ascending; the first k kept, padded.  The third key only matters
    when one (score, row) occurs in two parts: both copies come out, the earlier part's first (no de-duplication).
    On disjoint row sets this is tests/topk_ref.py::merge_topk (test_compose_cpu.py checks that).
    Planted defects: ``ties_by_part`` (equal scores ordered by position, not by row id), ``drop_equal`` (of two
    entries with equal scores only the first survives)."""
    parts, Q, k = scores.shape
    out_s, out_r = _padded(Q, k)
    for q in range(Q):
        s, r = scores[:, q, :].reshape(-1), rows[:, q, :].reshape(-1)
        pos = np.flatnonzero(r >= 0)
        s, r = s[pos], r[pos]
        order = np.lexsort((pos, pos if ties_by_part else r, -s))
        if drop_equal and order.size:
            so = s[order]
            order = order[np.concatenate([[True], so[1:] != so[:-1]])]
        order = order[:k]
        out_s[q, :order.size] = s[order]
        out_r[q, :order.size] = r[order]
    return out_s, out_r


def _over_queries(fn, q_bits: np.ndarray, work: int):
    """fn(query slice) -> tuple of arrays with the queries on axis 0; large jobs are split by QUERIES over a thread pool
    (ctypes releases the GIL; a query's answer does not depend on the other queries, so nothing has to be merged)."""
    Q = q_bits.shape[0]
    threads = min(THREADS, Q)
    if work < 5_000_000 or threads < 2:
        return fn(q_bits)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(threads) as ex:
        outs = list(ex.map(lambda idx: fn(np.ascontiguousarray(q_bits[idx])), np.array_split(np.arange(Q), threads)))
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(len(outs[0])))


def oracle_matrix(q_bits: np.ndarray, row_bits: np.ndarray, dtype: str) -> np.ndarray:
    """cref.cosine_matrix [Q,S] fp64."""
    work = q_bits.shape[0] * row_bits.shape[0] * q_bits.shape[1]
    return _over_queries(lambda q: (cref.cosine_matrix(q, row_bits, dtype=dtype),), q_bits, work)[0]


def oracle_topk(q_bits: np.ndarray, row_bits: np.ndarray, k: int, dtype: str, ids: Optional[np.ndarray] = None):
    """cref.cosine_topk in the library's (scores, rows) order; ``ids`` maps the oracle's positions to row ids.  No row
    at all: every entry -1 / 0.0."""
    Q = q_bits.shape[0]
    if row_bits.shape[0] == 0:
        return _padded(Q, k)
    work = Q * row_bits.shape[0] * q_bits.shape[1]
    r, s = _over_queries(lambda q: cref.cosine_topk(q, row_bits, k, dtype=dtype), q_bits, work)
    if ids is not None:
        r = np.where(r >= 0, np.asarray(ids, np.int64)[np.maximum(r, 0)], -1)
    return s, r


def chunk_starts(counts: Sequence[int]) -> np.ndarray:
    """int64 [F]: for every frame the first row of its own chunk within the group."""
    return np.repeat(np.cumsum([0] + list(counts[:-1])), counts).astype(np.int64)


def group_search_ref(mem_bits: np.ndarray, emb_bits: np.ndarray, counts: Sequence[int], k: int, dtype: str,
                     first_row: int = 0):
    """The definition the extractor claims (src/pipeline/vlm_extractor.py:44-74): for each chunk in turn,
    cosine_topk(chunk, everything stored so far, k), then the chunk is stored.  ``mem_bits`` are the stored rows in
    row-id order, the first of them row ``first_row``.  A chunk that finds nothing stored gets all -1 / 0.0."""
    F = emb_bits.shape[0]
    assert sum(counts) == F
    out_s, out_r = _padded(F, k)
    lo = 0
    for c in counts:
        if c:
            stored = np.concatenate([mem_bits, emb_bits[:lo]])
            s, r = oracle_topk(emb_bits[lo:lo + c], stored, k, dtype)
            out_s[lo:lo + c], out_r[lo:lo + c] = s, np.where(r >= 0, r + first_row, -1)
        lo += c
    return out_s, out_r


def group_search_composed(mem_bits, emb_bits, counts, k, dtype, first_row=0, *, group_base: Optional[int] = None,
                          select_kw: Optional[dict] = None, merge_kw: Optional[dict] = None):
    """What FrameEmbeddingExtractor._group_search computes, from the models above: top-k over the memory as it stands,
    select over the group's all-pairs matrix limited to the columns before each frame's chunk, merge of the two.
    ``group_base`` / ``select_kw`` / ``merge_kw`` plant defects."""
    s_mem, r_mem = oracle_topk(emb_bits, mem_bits, k, dtype)
    r_mem = np.where(r_mem >= 0, r_mem + first_row, -1)
    g = oracle_matrix(emb_bits, emb_bits, dtype)
    base = first_row + mem_bits.shape[0] if group_base is None else group_base
    s_grp, r_grp = select_ref(g, chunk_starts(counts), k, base, **(select_kw or {}))
    return merge_ref(np.stack([s_mem, s_grp]), np.stack([r_mem, r_grp]), **(merge_kw or {}))


def shard_live_ids(n_hist: int, world: int, counts: Optional[Sequence[int]] = None, cap: Optional[int] = None
                   ) -> List[np.ndarray]:
    """Per shard the global ids it can search, ascending.  Shard g received hist[g::world] (its first ``counts[g]``
    rows when given) and, as a ring of ``cap`` rows, keeps the last ``cap`` local ids; global id = local * world + g."""
    out = []
    for g in range(world):
        n = len(range(g, n_hist, world))
        if counts is not None:
            assert counts[g] <= n
            n = int(counts[g])
        lo = max(0, n - cap) if cap is not None else 0
        out.append(np.arange(lo, n, dtype=np.int64) * world + g)
    return out


def sharded_ref(q_bits, hist_bits, k, dtype, world, counts=None, cap=None):
    """Row-sharded retrieval by its plain definition: the oracle over the live rows in global-id order, mapped back to
    global ids (row i of ``hist_bits`` has global id i: it is local row i // world of shard i % world)."""
    ids = np.sort(np.concatenate(shard_live_ids(hist_bits.shape[0], world, counts, cap)))
    return oracle_topk(q_bits, hist_bits[ids], k, dtype, ids)


def shard_local(q_bits, hist_bits, k, dtype, world, counts=None, cap=None):
    """The W per-shard oracle lists with LOCAL row ids (scores [W,Q,k], local rows [W,Q,k], -1 padded): each shard's
    own live rows, nothing of the sharding in it yet.  A list at k is the first k columns of the list at any larger k
    (the order is total), which is how the tests share one oracle run among several k."""
    S, R = [], []
    for ids in shard_live_ids(hist_bits.shape[0], world, counts, cap):
        s, r = oracle_topk(q_bits, hist_bits[ids], k, dtype)          # r: position among the shard's live rows
        S.append(s)
        R.append(np.where(r >= 0, (ids[0] // world if ids.size else 0) + r, -1))
    return np.stack(S), np.stack(R)


def shard_global(local_rows: np.ndarray, n_hist: int, *, blocked_ids: bool = False, map_padding: bool = False):
    """Local rows [W,Q,k] -> global ids, local * world + rank.  Planted defects: ``blocked_ids`` (local + rank *
    n_local), ``map_padding`` (the -1 of a short shard's padding sent through the mapping like a row)."""
    W = local_rows.shape[0]
    out = np.empty_like(local_rows)
    for g in range(W):
        loc = local_rows[g]
        glob = loc + g * len(range(g, n_hist, W)) if blocked_ids else loc * W + g
        out[g] = glob if map_padding else np.where(loc >= 0, glob, -1)
    return out


def shard_parts(q_bits, hist_bits, k, dtype, world, counts=None, cap=None, **defect):
    """The W per-shard lists [W,Q,k] with strided global ids."""
    s, loc = shard_local(q_bits, hist_bits, k, dtype, world, counts, cap)
    return s, shard_global(loc, hist_bits.shape[0], **defect)


# ---------------------------------------------------------------------------------------------------------------------
# A. vm_cosine_exact operands
# ---------------------------------------------------------------------------------------------------------------------
COS16_D = (8, 24, 128, 1000, 4096)
COS32_D = (1, 7, 96, 1025)
COS_S = (0, 1, 255, 256, 257, 600)
COS_Q = (1, 3, 70)
# where the planted vectors sit: among the first rows (so that small S and Q still see some) and across the 256-row
# block edge; DUP holds one vector twice
PLANT_ZERO, PLANT_MAX, PLANT_SUB, PLANT_ONE, PLANT_DUP = 0, 1, 2, 3, (4, 5, 256)


def cosine_operands(dtype: str, D: int, seed: int, n: int = 600):
    """n vectors of length D with the plants above: uint16 [n, D] for f16 / bf16, float32 [n, D] for f32 whose random
    values are not representable in 16 bits (low mantissa bits set).  Row 6 is left random."""
    rng = np.random.default_rng(seed)
    if dtype == "f32":
        x = rng.standard_normal((n, D)).astype(np.float32)
        x = (x.view(np.uint32) | np.uint32(0x1001)).view(np.float32)     # beyond 11 and 8 mantissa bits
        x[PLANT_MAX] = np.finfo(np.float32).max
        sub = rng.integers(1, 0x800000, D, dtype=np.uint32) | (rng.integers(0, 2, D, dtype=np.uint32) << 31)
        x[PLANT_SUB] = sub.view(np.float32)                               # subnormal fp32: squares normal in fp64
        one = np.zeros(D, np.float32)
        one[D // 2] = x[7, D // 2]
        x[PLANT_ONE] = one
    else:
        x = to_bits(rng.standard_normal((n, D)), dtype)
        x[PLANT_MAX] = MAX_FINITE[dtype]
        sub = rng.integers(1, SUBNORMAL_MASK[dtype] + 1, D).astype(np.uint16)
        x[PLANT_SUB] = sub | (rng.integers(0, 2, D).astype(np.uint16) << 15)
        one = np.zeros(D, np.uint16)
        one[D // 2] = x[7, D // 2] | 0x0400 if dtype == "f16" else x[7, D // 2] | 0x0080   # never zero
        x[PLANT_ONE] = one
    x[PLANT_ZERO] = 0
    for p in PLANT_DUP[1:]:
        x[p] = x[PLANT_DUP[0]]
    return x


def cosine_pair(dtype: str, D: int):
    """(queries [70, D], rows [600, D]) of one (dtype, D): both operands carry every plant, and the two duplicate sets
    hold the same vector, so queries 4, 5 equal rows 4, 5, 256 (a query equal to a stored row)."""
    seed = 1000 * D + {"f16": 1, "bf16": 2, "f32": 3}[dtype]
    r = cosine_operands(dtype, D, seed)
    q = cosine_operands(dtype, D, seed + 7, n=70 + 187)[:70].copy()       # n > 256: the plant at 256 must exist
    for p in PLANT_DUP[:2]:
        q[p] = r[PLANT_DUP[0]]
    return q, r


# ---------------------------------------------------------------------------------------------------------------------
# B. vm_topk_select on crafted fp64 matrices
# ---------------------------------------------------------------------------------------------------------------------
SEL_S = (1, 255, 256, 257, 1000)
SEL_Q = (1, 5, 70)
SEL_K = (1, 4, 58, 300)
SEL_LIMITS = ("none", "zero", "S", "S+5", "-3", "mixed")
SEL_BASES = (0, 2 ** 40 + 7)
SEL_ROWS = ("random", "constant", "runs", "zeros", "inf", "ascending")


def select_row(kind: str, S: int, rng: np.random.Generator) -> np.ndarray:
    i = np.arange(S)
    if kind == "random":
        return rng.standard_normal(S)
    if kind == "constant":                       # pure column order
        return np.full(S, 0.25)
    if kind == "runs":                           # runs of 7 equal values: one straddles every column, 255 | 256 and any
        v = (i // 7 % 3) * 0.5                   # col_limit included; the best run of all straddles 255 | 256
        v[250:262] = 2.0
        return v
    if kind == "zeros":                          # +0.0 and -0.0 tie; the returned score keeps the entry's own bits
        return rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0]), S)
    if kind == "inf":                            # the kernel's sentinels are +-INFINITY: real ones must still rank
        v = rng.standard_normal(S)
        v[rng.random(S) < 0.2] = np.inf
        v[rng.random(S) < 0.2] = -np.inf
        return v
    assert kind == "ascending"                   # the best is the last admitted column
    return i * 1e-3 - 0.5


def select_matrix(S: int, Q: int) -> np.ndarray:
    """[Q,S] fp64: query q holds row kind (q + S) % 6, so Q = 5 and Q = 70 see (almost) every kind at every S and the
    single query of Q = 1 a different kind at every S."""
    rng = np.random.default_rng(77 * S + Q)
    return np.stack([select_row(SEL_ROWS[(q + S) % len(SEL_ROWS)], S, rng) for q in range(Q)])


def select_limit(kind: str, S: int, Q: int) -> Optional[np.ndarray]:
    if kind == "none":
        return None
    if kind == "mixed":
        cyc = [0, 1, S - 1, S, S // 2, 255, 256, S + 5, -3, 3]
        return np.array([cyc[q % len(cyc)] for q in range(Q)], np.int64)
    return np.full(Q, {"zero": 0, "S": S, "S+5": S + 5, "-3": -3}[kind], np.int64)


def select_cases(S_values=SEL_S):
    """Every (S, Q, k, col_limit kind, row_base) -> (id, scores, col_limit, k, row_base)."""
    for S, Q in itertools.product(S_values, SEL_Q):
        m = select_matrix(S, Q)
        for k, lim, base in itertools.product(SEL_K, SEL_LIMITS, SEL_BASES):
            yield f"S{S}-Q{Q}-k{k}-lim{lim}-base{base}", m, select_limit(lim, S, Q), k, base


# ---------------------------------------------------------------------------------------------------------------------
# C. vm_topk_merge on crafted lists
# ---------------------------------------------------------------------------------------------------------------------
MRG_PARTS = (1, 2, 3, 8)
MRG_K = (1, 4, 58, 300)
MRG_Q = (1, 5, 70)
MRG_KINDS = ("full", "some-empty", "all-empty", "ragged", "late-part-small-row", "few-live", "big-ids", "shared")


def merge_query(kind: str, parts: int, k: int, rng: np.random.Generator):
    """One query's lists (scores [parts,k], rows [parts,k]), each sorted (score desc, row asc) and -1 / 0.0 padded:
      full                 every part full, random scores, disjoint strided rows
      some-empty           the odd parts hold nothing
      all-empty            no part holds anything
      ragged               parts padded to different lengths
      late-part-small-row  scores from {0, 1/4, 1/2, 3/4}: ties within a part and across parts, and at equal rank the
                           LATER part holds the SMALLER row id
      few-live             fewer than k live entries in all
      big-ids              tied scores again, row ids on both sides of 2**40
      shared               the last part repeats every other entry of part 0, (score, row) and all: not what a caller
                           should pass (shards are disjoint), pinned as the kernel does it - both copies come out
    """
    lens = [k] * parts
    if kind == "some-empty":
        lens = [k if p % 2 == 0 else 0 for p in range(parts)]
    elif kind == "all-empty":
        lens = [0] * parts
    elif kind == "ragged":
        lens = [(p * 37 + 11) % (k + 1) for p in range(parts)]
    elif kind == "few-live":
        lens = [(k // 2) // parts + (1 if p < (k // 2) % parts else 0) for p in range(parts)]
    base = 2 ** 40 - 5 if kind == "big-ids" else 0
    tied = kind in ("late-part-small-row", "big-ids", "shared")
    lists = []
    for p in range(parts):
        n = lens[p]
        ids = base + np.arange(n, dtype=np.int64) * parts + (parts - 1 - p if kind == "late-part-small-row" else p)
        sc = rng.integers(0, 4, n) / 4.0 if tied else rng.standard_normal(n)
        lists.append((sc, ids))
    if kind == "shared" and parts >= 2:
        sc0, id0 = lists[0]
        sc, ids = lists[-1]
        m = (k + 1) // 2
        lists[-1] = (np.concatenate([sc0[::2], sc[m:]]), np.concatenate([id0[::2], ids[m:]]))
    s, r = np.zeros((parts, k)), np.full((parts, k), -1, np.int64)
    for p, (sc, ids) in enumerate(lists):
        order = np.lexsort((ids, -sc))
        s[p, :order.size], r[p, :order.size] = sc[order], ids[order]
    return s, r


def merge_lists(parts: int, k: int, Q: int):
    """[parts,Q,k] lists: query q holds kind (q + parts + k) % 8 (Q = 70 sees every kind at every shape)."""
    rng = np.random.default_rng(parts * 1009 + k * 31 + Q)
    per_q = [merge_query(MRG_KINDS[(q + parts + k) % len(MRG_KINDS)], parts, k, rng) for q in range(Q)]
    return np.stack([x[0] for x in per_q], axis=1), np.stack([x[1] for x in per_q], axis=1)


def merge_cases():
    for parts, k, Q in itertools.product(MRG_PARTS, MRG_K, MRG_Q):
        yield (f"parts{parts}-k{k}-Q{Q}",) + merge_lists(parts, k, Q)


def merge_signed_zero_case():
    """The same row with score +0.0 in part 0 and -0.0 in part 1 (they tie, and the rows tie): the only input on which
    'earlier part first' can be seen in the output bits.  -> (scores [2,1,2], rows [2,1,2])."""
    s = np.array([[[0.0, -1.0]], [[-0.0, -2.0]]])
    r = np.array([[[5, 9]], [[5, 3]]], np.int64)
    return s, r


# ---------------------------------------------------------------------------------------------------------------------
# D. sharded retrieval
# ---------------------------------------------------------------------------------------------------------------------
SHARD_W = (3, 8)
SHARD_TYPES = (("f16", 256), ("bf16", 128))
SHARD_K = (1, 10, 58, 100)                    # 100: the all-query exhaustive route (k > 58)
SHARD_KMAX = max(SHARD_K)
SHARD_M = (5,) + tuple(8 * k - 3 for k in SHARD_K[1:]) + (1000, 20_011)   # 8 k - 3 at k = 1 is the 5 already there
SHARD_Q = 24


@dataclass
class ShardCase:
    name: str
    dtype: str
    D: int
    world: int
    hist: np.ndarray                 # uint16 [M, D]: row i has global id i and lives on shard i % world
    queries: np.ndarray              # uint16 [Q, D]
    ks: Tuple[int, ...]
    expect: dict                     # query -> the first global ids its answer must start with (the plants)
    cap: Optional[int] = None        # ring shards of this capacity
    capacity: Optional[int] = None   # a linear shard's capacity (default: just above its rows)
    steps: Optional[List[List[int]]] = None   # ring: rows every shard has received after each append step


def plant_shards(hist: np.ndarray, queries: np.ndarray, world: int) -> dict:
    """Plants, where the memory is large enough to hold them:
      query 0  an exact duplicate pair on two different shards, the LARGER id on the LOWER rank
      query 1  a run of 2 W + 4 identical rows: consecutive global ids, so it rotates through every shard; the answer
               is the lowest ids of the run
      query 2  the zero query (every score 0.0: the lowest ids of the memory)
      query 3  equal to one stored row (and a zero row sits in the memory)
    -> {query: first expected global ids}"""
    M, W = hist.shape[0], world
    expect = {}
    queries[2] = 0
    expect[2] = list(range(M))
    if M >= 64:
        a, b = 2 * W - 1, W * (M // W - 1)       # ranks W - 1 and 0, a < b
        hist[b] = hist[a]
        queries[0] = hist[a]
        expect[0] = [a, b]
        r0, L = M // 2, 2 * W + 4
        hist[r0:r0 + L] = hist[r0]
        queries[1] = hist[r0]
        expect[1] = list(range(r0, r0 + L))
        hist[M // 3] = 0
        queries[3] = hist[M // 4]
        expect[3] = [M // 4]
    elif M > W:                                   # rows W - 1 (rank W - 1) and W (rank 0)
        hist[W] = hist[W - 1]
        queries[0] = hist[W]
        expect[0] = [W - 1, W]
    elif M >= 2:                                  # fewer rows than shards: the pair sits on ranks 0 and M - 1
        hist[M - 1] = hist[0]
        queries[0] = hist[0]
        expect[0] = [0, M - 1]
    return expect


def _shard_case(name, dtype, D, W, M, ks, seed, Q=SHARD_Q, **kw) -> ShardCase:
    rng = np.random.default_rng(seed)
    hist, queries = unit_bits(rng, M, D, dtype), unit_bits(rng, Q, D, dtype)
    return ShardCase(name, dtype, D, W, hist, queries, tuple(ks), plant_shards(hist, queries, W), **kw)


def shard_cases() -> List[ShardCase]:
    """W x type x M, every k on each: M = 5 leaves shards with no row at all, M = 8 k - 3 every shard shorter than k."""
    out = []
    for W, (dtype, D), M in itertools.product(SHARD_W, SHARD_TYPES, SHARD_M):
        out.append(_shard_case(f"W{W}-{dtype}-D{D}-M{M}", dtype, D, W, M, SHARD_K, seed=W * 100_003 + D + M))
    return out


def dist_worker_case() -> ShardCase:
    """tests/dist_worker.py's figures per shard at W = 8: 3,000 f16 rows of D = 256 per shard, 20 identical rows on
    every shard (160 consecutive global ids), k = 7: each shard's scan cannot certify the tie and redoes the query."""
    c = _shard_case("dist-worker-W8", "f16", 256, 8, 24_000, (7,), seed=5)
    c.hist[1000:1160] = c.hist[1000]
    for q in (5, 15):
        c.queries[q] = c.hist[1000]
        c.expect[q] = list(range(1000, 1160))
    return c


RING_CAP, RING_FED = 96, 250
RING_APPENDS = (1, 37, 58, 96, 7, 51)          # sums to RING_FED; shard g takes them rotated by g


def ring_case() -> ShardCase:
    """W = 8 ring shards of capacity 96, 250 rows each in uneven appends (uneven across the shards too), searched
    after every append step: the strided ids of rings that are empty, filling, exactly full and wrapped."""
    assert sum(RING_APPENDS) == RING_FED
    W = 8
    c = _shard_case("ring-W8", "bf16", 128, W, W * RING_FED, (10,), seed=96, cap=RING_CAP)
    n = len(RING_APPENDS)
    got, steps = [0] * W, []
    for t in range(n):
        got = [got[g] + RING_APPENDS[(t + g) % n] for g in range(W)]
        steps.append(list(got))
    c.steps = steps
    c.expect = {}                                # the plants of the full history are not live at every step
    return c


CASCADE_CAP, CASCADE_Q, CASCADE_K = 65_536, 64, 20


def cascade_case() -> ShardCase:
    """The strided mapping on the emit cascade: launches are sized from the CAPACITY (65,536 rows of D = 128, 16 MB a
    shard), so 3,000 rows per shard suffice; 64 queries, k = 20 (tests/topk_plan.py: family 'cascade')."""
    return _shard_case("cascade-W8", "f16", 128, 8, 8 * 3000 + 5, (CASCADE_K,), seed=65_536, Q=CASCADE_Q,
                       capacity=CASCADE_CAP)


def all_shard_cases() -> List[ShardCase]:
    return shard_cases() + [dist_worker_case(), ring_case(), cascade_case()]


# ---------------------------------------------------------------------------------------------------------------------
# E. the look-ahead group search
# ---------------------------------------------------------------------------------------------------------------------
GRP_TYPES = (("f16", 768), ("bf16", 1024), ("f16", 128), ("bf16", 128))
GRP_MEMS = ("empty", "short", "filled", "ring-to-capacity")
GRP_COUNTS = ((7, 7, 7), (7, 7, 3), (5, 0, 7, 1), (15,) * 20, (1,))
GRP_K = (1, 4, 20, 58, 64)                     # 64: memory.topk takes its exhaustive route
GRP_CONTENTS = ("random", "static", "repeat", "zero")
GRP_GROUPS = 3


@dataclass
class GroupCase:
    name: str
    dtype: str
    D: int
    mem_kind: str
    counts: Tuple[int, ...]
    k: int
    mem: np.ndarray                  # uint16 [n0, D]: the rows stored before the first group
    groups: List[np.ndarray]         # three groups' embeddings, uint16 [F, D] each
    contents: Tuple[str, ...]

    @property
    def capacity(self) -> int:
        return max(1, self.mem.shape[0] + sum(g.shape[0] for g in self.groups)) + (0 if self.ring else 9)

    @property
    def ring(self) -> bool:
        return self.mem_kind == "ring-to-capacity"


def group_content(kind: str, rng, counts, D, dtype, scene: np.ndarray, stored: np.ndarray) -> np.ndarray:
    """One group's embeddings [F, D]:
      random  unit rows
      static  every frame the scene vector, which several stored rows hold too (a static camera): the answer is the
              lowest ids, memory first, and no frame may find itself or its own chunk
      repeat  the first frame of the third non-empty chunk equals the first frame of the first chunk and one stored row
      zero    a zero embedding in the middle of the group (the memory holds a zero row as well)
    """
    F = sum(counts)
    emb = unit_bits(rng, F, D, dtype)
    if kind == "static":
        emb[:] = scene
    elif kind == "repeat":
        starts = [s for s, c in zip(np.cumsum([0] + list(counts[:-1])), counts) if c]
        if stored.shape[0]:
            emb[0] = stored[stored.shape[0] // 2]
        if len(starts) >= 3:
            emb[starts[2]] = emb[0]
        else:
            emb[F - 1] = emb[0]
    elif kind == "zero":
        emb[F // 2] = 0
    return emb


def _group_case(i_t, i_m, i_c) -> GroupCase:
    (dtype, D), mem_kind, counts = GRP_TYPES[i_t], GRP_MEMS[i_m], GRP_COUNTS[i_c]
    # every k and every first content meets every memory kind and every counts (Latin squares over the two indices)
    k = GRP_K[(i_m + i_c + i_t) % len(GRP_K)]
    c0 = (i_m + 2 * i_c + i_t) % len(GRP_CONTENTS)
    contents = tuple(GRP_CONTENTS[(c0 + j) % len(GRP_CONTENTS)] for j in range(GRP_GROUPS))
    rng = np.random.default_rng(10_000 * i_t + 100 * i_m + i_c)
    n0 = {"empty": 0, "short": min(k - 1, 3), "filled": 300 + 17 * i_c, "ring-to-capacity": 150}[mem_kind]
    mem = unit_bits(rng, n0, D, dtype)
    scene = unit_bits(rng, 1, D, dtype)[0]
    if n0 >= 100:
        for p in (3, 40, 41, n0 - 1):
            mem[p] = scene
        mem[n0 // 3] = 0
    elif n0:
        mem[n0 - 1] = scene
    groups, stored = [], mem
    for kind in contents:
        emb = group_content(kind, rng, counts, D, dtype, scene, stored)
        groups.append(emb)
        stored = np.concatenate([stored, emb])
    name = f"{dtype}-D{D}-{mem_kind}-counts{'x'.join(map(str, counts[:4]))}{'..' if len(counts) > 4 else ''}-k{k}"
    return GroupCase(name, dtype, D, mem_kind, tuple(counts), k, mem, groups, contents)


def group_cases() -> List[GroupCase]:
    """types x memories x counts.  The 300-frame group (20 chunks of 15) meets D = 768 / 1024 on the filled memory only
    and every memory kind at D = 128: the oracle's time goes with F * rows * D, and what F = 300 adds - a second
    256-column block in the all-pairs and the select kernel - does not depend on D."""
    return [_group_case(i_t, i_m, i_c) for i_t in range(len(GRP_TYPES)) for i_m in range(len(GRP_MEMS))
            for i_c in range(len(GRP_COUNTS))
            if not (sum(GRP_COUNTS[i_c]) > 256 and GRP_TYPES[i_t][1] > 128 and GRP_MEMS[i_m] != "filled")]


def group_walk(c: GroupCase):
    """The running model: yields (stored rows before the group, the group's embeddings) for the three groups."""
    stored = c.mem
    for emb in c.groups:
        yield stored, emb
        stored = np.concatenate([stored, emb])
