"""One host model of the whole memory (include/vidmem.h), numpy only.

Every feature of the memory has its own oracle; this file composes them into ONE model that is carried through a whole
life - keyed, tagged and gated appends, erases, whole and tail regroups, the ring overwrite, reset, snapshot / restore -
and says after every step what all nine readers must return (torch only where the existing data generators use it,
``pool`` and ``noisy``).  It defines no cosine and no ranking of its own: every
mutator restates the header's rule by calling the oracle that already states it (novelty_ref.gate, erase_ref.erase,
events_ref.regroup / regroup_tail), every expectation is the feature's own oracle over the live window.

``Model``       the state, in row-id order, and the mutators.
``checkpoint``  compares an ``EmbeddingMemory`` (or anything with its surface) with the model through the public
                accessors and all nine readers, each top-k reader in its default and its ``exact`` form; bit equality.
``Driver``      applies one step to the model and to the memory, compares what the step returns, builds the probes.
``linear_script`` / ``ring_script``  the two lives of tests/test_lifecycle_gpu.py; tests/test_lifecycle_cpu.py runs the
                same scripts against a fake memory, proves the conditions they must meet and plants defects.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from oracle import cref
from tests import clip_ref as CL
from tests import erase_ref as E
from tests import events_ref as V
from tests import group_ref as G
from tests import group_scope_ref as GS
from tests import novelty_ref as N
from tests import range_ref as R
from tests import scope_ref as S
from tests import summary_ref as M

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
SCOPE_ALL = (INT64_MIN, INT64_MAX)
MS_BITS = 40
MS = 33                       # milliseconds between two frames of one source
K = 5
MAX_HITS = 64
THRESHOLD, GAP_MS = 0.5, 2000  # the events / regroup arguments of both scripts
DIMS = {"f16": 128, "bf16": 256}
VM_ERR_UNSUPPORTED = -4                # include/vidmem.h vm_status


def make_tag(source, ms):
    return (int(source) << MS_BITS) | int(ms)


class Window(NamedTuple):
    rows: np.ndarray       # uint16 [n, D]
    tags: np.ndarray       # int64 [n]
    keys: np.ndarray       # int64 [n]
    ords: np.ndarray       # int64 [n] group ordinals as the device counts them
    ids: list              # str per row
    prov: np.ndarray       # int64 [n] index of the source row in the data pool


class Probes(NamedTuple):
    queries: np.ndarray    # uint16 [6, D]
    scopes: list           # six (lo, hi)
    clips: list            # uint16 [1, L, D] each
    range_min: float
    k: int = K
    max_hits: int = MAX_HITS
    threshold: float = THRESHOLD
    gap_ms: int = GAP_MS


class Model:
    """Rows, tags, keys, ordinals, ids and provenance of every row appended since the last reset or erase renumbering,
    in row-id order; ``state`` = (groups opened, last key, open); ``used`` = slots a linear memory has written since the
    last reset (an erase zeroes what it vacates, a reset promises nothing about the columns)."""

    def __init__(self, D, dtype, capacity, ring=False):
        self.D, self.dtype, self.capacity, self.ring = int(D), dtype, int(capacity), bool(ring)
        self.reset()

    # ---- state ---------------------------------------------------------------------------------------------------
    def reset(self):
        self.rows = np.zeros((0, self.D), np.uint16)
        self.tags = np.zeros(0, np.int64)
        self.keys = np.zeros(0, np.int64)
        self.ords = np.zeros(0, np.int64)
        self.prov = np.zeros(0, np.int64)
        self.ids = []
        self.state = (0, 0, 0)
        self.used = 0

    @property
    def total(self):
        return self.rows.shape[0]

    @property
    def base(self):
        return max(0, self.total - self.capacity) if self.ring else 0

    @property
    def wrapped(self):
        return self.ring and self.total > self.capacity

    def window(self):
        """(base, the live columns): what a search sees, as novelty_ref.GatedMemory.window."""
        lo = self.base
        return lo, Window(self.rows[lo:], self.tags[lo:], self.keys[lo:], self.ords[lo:], self.ids[lo:], self.prov[lo:])

    # ---- mutators ------------------------------------------------------------------------------------------------
    def append(self, rows, tags, keys, ids, prov=None):
        """vm_memory_append_tagged with keys: the first row continues the open group iff the state is open and its key
        is the last key; then a row opens a group when its key differs from the row before it."""
        rows = np.asarray(rows, np.uint16).reshape(-1, self.D)
        B = rows.shape[0]
        if B == 0:
            return self.total
        keys = np.asarray(keys, np.int64).reshape(-1)
        groups, last, is_open = self.state
        flags = np.ones(B, bool)
        flags[0] = not (is_open and int(keys[0]) == last)
        flags[1:] = keys[1:] != keys[:-1]
        first = self.total
        self.rows = np.concatenate([self.rows, rows])
        self.tags = np.concatenate([self.tags, np.asarray(tags, np.int64).reshape(-1)])
        self.keys = np.concatenate([self.keys, keys])
        self.ords = np.concatenate([self.ords, groups + np.cumsum(flags) - 1]).astype(np.int64)
        self.prov = np.concatenate([self.prov, np.full(B, -1, np.int64) if prov is None else np.asarray(prov, np.int64)])
        self.ids = self.ids + list(ids)
        self.state = (groups + int(flags.sum()), int(keys[-1]), 1)
        if not self.ring:
            self.used = max(self.used, self.total)
        return first

    def known(self, batch):
        lo, live = self.window()
        return N.top1(batch, live.rows, self.dtype, base=lo)

    def append_novel(self, batch, tau, tags, keys, ids, prov=None, known=None):
        """vm_memory_append_novel with ``known`` = topk(batch, 1) over the window (novelty_ref.top1), then the kept rows
        as one keyed, tagged append; a call that keeps nothing leaves everything untouched."""
        batch = np.asarray(batch, np.uint16).reshape(-1, self.D)
        ks, kr = self.known(batch) if known is None else known
        keep, row_of = N.gate(batch, tau, self.dtype, self.total, ks, kr)
        if keep.any():
            prov = None if prov is None else np.asarray(prov, np.int64)[keep]
            self.append(batch[keep], np.asarray(tags, np.int64)[keep], np.asarray(keys, np.int64)[keep],
                        [i for i, kp in zip(ids, keep) if kp], prov)
        return keep, row_of

    def _erase(self, drop):
        if self.wrapped:
            return None                                    # refused: VM_ERR_UNSUPPORTED, nothing changes
        out = E.erase(E.Columns(self.rows, self.tags, self.keys), drop)
        keep = ~np.asarray(drop, bool)
        self.rows, self.tags, self.keys = out.cols.rows, out.cols.tags, out.cols.keys
        self.ords, self.state = out.ordinals, out.state
        self.prov = self.prov[keep]
        self.ids = [i for i, kp in zip(self.ids, keep) if kp]
        return out

    def erase_rows(self, ids):
        return self._erase(E.mask_of_rows(self.total, ids))

    def erase_scopes(self, scopes):
        return self._erase(E.mask_of_scopes(self.tags, scopes))

    def flags(self, threshold, gap_ms):
        """(base, bool [n]): which live rows open an event (events_ref.links / opens over the window)."""
        lo, live = self.window()
        return lo, V.opens(V.links(live.rows, self.dtype), threshold, live.tags, gap_ms)

    def regroup_whole(self, threshold, gap_ms):
        if self.total == 0:
            return 0
        lo, flags = self.flags(threshold, gap_ms)
        out = V.regroup(flags, lo)
        self.keys = np.concatenate([self.keys[:lo], out.keys])
        self.ords = np.concatenate([self.ords[:lo], out.ordinals])
        self.state = out.state
        return out.state[0]

    def regroup_tail(self, threshold, gap_ms, from_row):
        if from_row <= self.base:
            return self.regroup_whole(threshold, gap_ms)
        if from_row >= self.total:
            return 0
        lo, flags = self.flags(threshold, gap_ms)
        out = V.regroup_tail(self.keys[lo:], self.ords[lo:], flags, from_row - lo, lo)
        self.keys = np.concatenate([self.keys[:lo], out.keys])
        self.ords = np.concatenate([self.ords[:lo], out.ordinals])
        self.state = out.state
        return int(flags[from_row - lo:].sum())

    def restored(self, capacity=None, ring=False):
        """The model of ``EmbeddingMemory.restore(snapshot)``: the live window renumbered from 0 in one keyed, tagged
        append - ordinals re-derived from the keys, the state open with the last key."""
        _, live = self.window()
        out = Model(self.D, self.dtype, capacity or max(live.rows.shape[0], 1), ring)
        out.append(live.rows, live.tags, live.keys, live.ids, live.prov)
        return out

    # ---- expectations: each reader's own oracle over the window ----------------------------------------------------
    def exp_topk(self, q, k):
        lo, live = self.window()
        if live.rows.shape[0] == 0:
            return np.full((q.shape[0], k), -1, np.int64), np.zeros((q.shape[0], k))
        r, s = cref.cosine_topk(np.ascontiguousarray(q), np.ascontiguousarray(live.rows), k, dtype=self.dtype)
        return np.where(r >= 0, r + lo, -1), s

    def exp_grouped(self, q, k):
        lo, live = self.window()
        if live.rows.shape[0] == 0:
            return np.full((q.shape[0], k), -1, np.int64), np.zeros((q.shape[0], k)), np.full((q.shape[0], k), -1, np.int64)
        return G.grouped_topk(q, np.ascontiguousarray(live.rows), live.keys, k, dtype=self.dtype, base=lo)

    def exp_scoped(self, q, scopes, k):
        lo, live = self.window()
        return S.scoped_topk(q, live.rows, live.tags, scopes, k, dtype=self.dtype, base=lo)

    def exp_grouped_scoped(self, q, scopes, k):
        lo, live = self.window()
        if live.rows.shape[0] == 0:
            return self.exp_grouped(q, k)
        return GS.group_scoped_topk(q, np.ascontiguousarray(live.rows), live.keys, live.tags, scopes, k,
                                    dtype=self.dtype, base=lo)

    def exp_clip(self, clips, k):
        lo, live = self.window()
        return CL.clip_topk(clips, live.rows, k, clips.shape[1], dtype=self.dtype, tags=live.tags, base=lo)

    def exp_range(self, q, min_score, scopes):
        lo, live = self.window()
        if live.rows.shape[0] == 0:
            return [(np.zeros(0, np.int64), np.zeros(0), 0) for _ in range(q.shape[0])]
        return R.range_hits(q, live.rows, min_score, live.tags, scopes, dtype=self.dtype, base=lo)

    def exp_events(self, threshold, gap_ms):
        lo, live = self.window()
        return V.events(live.rows, threshold, self.dtype, live.tags, gap_ms, lo)

    def exp_summaries(self):
        lo, live = self.window()
        return M.summarize(live.rows, live.keys, self.dtype, lo)

    def expect(self, p: Probes):
        return {"topk": self.exp_topk(p.queries, p.k), "grouped": self.exp_grouped(p.queries, p.k),
                "scoped": self.exp_scoped(p.queries, p.scopes, p.k),
                "grouped_scoped": self.exp_grouped_scoped(p.queries, p.scopes, p.k),
                "clip": [self.exp_clip(c, p.k) for c in p.clips],
                "range": self.exp_range(p.queries, p.range_min, p.scopes),
                "events": self.exp_events(p.threshold, p.gap_ms), "summaries": self.exp_summaries()}


# ---- checkpoint --------------------------------------------------------------------------------------------------------
def _np(x):
    """A device tensor, a host tensor or an array -> numpy."""
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(_np(a), np.float64), np.ascontiguousarray(np.asarray(b), np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _same(got, want, what):
    assert np.array_equal(_np(got), np.asarray(want)), f"{what}: {_np(got).tolist()} != {np.asarray(want).tolist()}"


UNCERT = ("uncertified_count", "grouped_uncertified_count", "scoped_uncertified_count",
          "group_scoped_uncertified_count", "clip_uncertified_count")


def checkpoint(mem, model: Model, p: Probes, io, exp=None, label=""):
    """``mem`` against ``model``: the accessors, then the nine readers; -> the ``*_uncertified_count`` of every reader.
    ``io`` carries what is not part of the memory's surface: ``t(bits)`` (bit patterns -> what the memory takes as
    rows), ``ordinals(mem)`` (the ordinal column of the live rows in row-id order, vm_memory_group_ordinals) and
    ``raw(mem, n)`` (rows, tags, keys, ordinals over slots [0, n) in slot order)."""
    exp = model.expect(p) if exp is None else exp
    lo, live = model.window()
    n = live.rows.shape[0]
    at = f"[{label}] "
    assert len(mem) == model.total, f"{at}len {len(mem)} != {model.total}"
    assert mem.searchable == n, f"{at}searchable {mem.searchable} != {n}"
    got_lo, got_rows = mem.rows_host()
    assert got_lo == lo, f"{at}first live row {got_lo} != {lo}"
    assert np.array_equal(got_rows, live.rows), f"{at}rows_host differs"
    _same(mem.tags_host(), live.tags, at + "tags_host")
    _same(mem.group_keys_host(), live.keys, at + "group_keys_host")
    ords = np.asarray(io.ordinals(mem), np.int64)
    assert ords.shape == (n,), f"{at}{ords.shape[0]} ordinals for {n} live rows"
    if n:
        _same(ords - ords[0], live.ords - live.ords[0], at + "ordinals relative to the first live row")
    for i in range(n):
        assert mem.id_of(lo + i) == live.ids[i], f"{at}id_of({lo + i}) = {mem.id_of(lo + i)!r}, want {live.ids[i]!r}"
        assert mem.meta_of(lo + i) == {"i": live.ids[i]}, f"{at}meta_of({lo + i}) = {mem.meta_of(lo + i)!r}"
    assert mem.id_of(lo - 1) is None, f"{at}id_of({lo - 1}) = {mem.id_of(lo - 1)!r}: a row that is not live has an id"
    assert mem.id_of(model.total) is None, f"{at}id_of(one past the end) is not None"
    assert mem.meta_of(lo - 1) is None and mem.meta_of(model.total) is None, f"{at}meta_of of a row that is not live"
    if not model.ring:      # every slot ever used: the live rows, then zeros (forgetting means the bytes are gone)
        raw = io.raw(mem, model.used)
        for name, col, want in zip(("rows", "tags", "keys", "ordinals"), raw, (live.rows, live.tags, live.keys, live.ords)):
            col = np.asarray(col)
            assert np.array_equal(col[:n], want), f"{at}raw {name} of the live slots differ"
            assert not col[n:].any(), f"{at}raw {name}: a slot past the live count is not zero"

    q = io.t(p.queries)
    for exact in (False, True):
        form = f"{at}{'exact' if exact else 'default'} "
        s, r = mem.topk(q, p.k, exact=exact)
        _same(r, exp["topk"][0], form + "topk rows")
        assert _bits_equal(s, exp["topk"][1]), form + "topk scores (bit-exact bar)"
        s, r, kk = mem.topk_grouped(q, p.k, exact=exact)
        _same(r, exp["grouped"][0], form + "topk_grouped rows")
        _same(kk, exp["grouped"][2], form + "topk_grouped keys")
        assert _bits_equal(s, exp["grouped"][1]), form + "topk_grouped scores"
        s, r = mem.topk_scoped(q, p.k, p.scopes, exact=exact)
        _same(r, exp["scoped"][0], form + "topk_scoped rows")
        assert _bits_equal(s, exp["scoped"][1]), form + "topk_scoped scores"
        s, r, kk = mem.topk_grouped_scoped(q, p.k, p.scopes, exact=exact)
        _same(r, exp["grouped_scoped"][0], form + "topk_grouped_scoped rows")
        _same(kk, exp["grouped_scoped"][2], form + "topk_grouped_scoped keys")
        assert _bits_equal(s, exp["grouped_scoped"][1]), form + "topk_grouped_scoped scores"
        for clip, want in zip(p.clips, exp["clip"]):
            s, r = mem.topk_clip(io.t(clip), p.k, exact=exact)
            _same(r, want[0], form + f"topk_clip L={clip.shape[1]} rows")
            assert _bits_equal(s, want[1]), form + f"topk_clip L={clip.shape[1]} scores"
        hits = mem.range_search(q, p.range_min, scope=p.scopes, max_hits=p.max_hits, exact=exact)
        want_r, want_s, want_c = R.padded(exp["range"], p.max_hits)
        assert len(hits) == len(exp["range"])
        for i, h in enumerate(hits):
            w = min(int(want_c[i]), p.max_hits)
            assert h.count == want_c[i], f"{form}range_search count of query {i}: {h.count} != {want_c[i]}"
            _same(h.rows, want_r[i, :w], form + f"range_search rows of query {i}")
            assert _bits_equal(h.scores, want_s[i, :w]), form + f"range_search scores of query {i}"
    link, seg = exp["events"]
    ev = mem.events(p.threshold, max_gap_ms=p.gap_ms, with_links=True)
    assert ev.count == seg.count, f"{at}events count {ev.count} != {seg.count}"
    _same(ev.first_rows, seg.first_rows, at + "events first_rows")
    _same(ev.event_of, seg.event_of, at + "events event_of")
    assert _bits_equal(ev.links, link), at + "events links"
    want = exp["summaries"]
    sm = mem.summaries()
    assert sm.count == want.first_rows.size, f"{at}summaries count {sm.count} != {want.first_rows.size}"
    _same(sm.first_rows, want.first_rows, at + "summaries first_rows")
    _same(sm.n_rows, want.n_rows, at + "summaries n_rows")
    _same(sm.keys, want.keys, at + "summaries keys")
    _same(io.bits(sm.centroids), want.centroids, at + "summaries centroids")
    _same(sm.key_rows, want.key_rows, at + "summaries key_rows")
    assert _bits_equal(sm.key_scores, want.key_scores), at + "summaries key_scores"
    return {name: int(getattr(mem, name)) for name in UNCERT}


# ---- data ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool(dtype):
    """(row bits uint16 [P, D], scene index [P]) of one dtype, made on the CPU once per process and never modified:
    planted scenes of ragged sizes 1 - 23 (tests/test_group_topk_gpu.clustered, noise 0.3: rows of one scene score about
    0.92 against each other, rows of two scenes about 0).  f16: every row scaled by 2^u, u uniform in [-2, 2], so the
    row norms spread over a factor of 16 and a norm left on the wrong row shows (tests/test_erase_gpu._data); bf16:
    unit rows."""
    import torch
    from tests.test_group_topk_gpu import _sizes, clustered
    D = DIMS[dtype]
    sizes = _sizes(330, "ragged", 11 if dtype == "f16" else 12)
    rows, gid = clustered(sizes, D, "f16" if dtype == "f16" else "bf16", seed=201 if dtype == "f16" else 202, noise=0.3,
                          device="cpu")
    x = rows.float().numpy()
    if dtype == "f16":
        x = x * (2.0 ** np.random.default_rng(7).uniform(-2, 2, size=(x.shape[0], 1))).astype(np.float32)
    bits = CL.to_bits(x, dtype)
    bits.setflags(write=False)
    scene = gid.numpy().astype(np.int64)
    scene.setflags(write=False)
    return bits, scene


def noisy(bits, dtype, seed, noise=0.1):
    """Bit patterns -> the same rows plus ``noise`` x their norm x unit noise, rounded to the dtype."""
    x = CL.from_bits(np.ascontiguousarray(bits), dtype).astype(np.float64)
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(x.shape)
    e /= np.linalg.norm(e, axis=-1, keepdims=True)
    return CL.to_bits((x + noise * np.linalg.norm(x, axis=-1, keepdims=True) * e).astype(np.float32), dtype)


def outside_row(D, seed=99):
    """One bf16 row of norm 2^45: outside the certificate's domain [2^-40, 2^40], so the memory's sticky word is set."""
    v = np.random.default_rng(seed).standard_normal(D)
    return CL.to_bits((v / np.linalg.norm(v) * 2.0 ** 45).astype(np.float32)[None, :], "bf16")


# ---- driver ----------------------------------------------------------------------------------------------------------------
class Driver:
    """One step at a time on the model and on the memory; what a step returns is compared at once, everything else at
    the next ``check``.  Rows come from ``pool(dtype)`` in order (``take``), so every stored row has a provenance."""

    def __init__(self, mem, model: Model, io, hooks=()):
        self.mem, self.model, self.io, self.hooks = mem, model, io, list(hooks)
        self.dtype = model.dtype
        self.bits, self.scene = pool(model.dtype)
        self.cursor = 0
        self.clock = {}                  # source -> frames appended so far
        self.log = []                    # (label, uncertified counts)
        self.gated = []                  # kept fraction of every gated batch
        self.src = []                    # the bits every stored row came from; a row's provenance is its index here
        self.moved = self.gone = self.overwritten = None       # provenances for the probes
        self.join = None                 # live row index where an erase made two rows adjacent
        self.seq = 0
        self.stored = 0                  # rows that ever became live
        self.restored = []               # the drivers ``restore`` made: their memories are the caller's to close

    # -- data
    def take(self, n):
        """The next ``n`` pool rows -> their pool indices."""
        idx = np.arange(self.cursor, self.cursor + n)
        assert idx[-1] < self.bits.shape[0], "the data pool is used up"
        self.cursor += n
        return idx

    def take_scenes(self, n):
        """Whole scenes from the cursor on, at least ``n`` rows (the cursor must stand at a scene's first row)."""
        end = self.cursor + n
        while self.scene[end] == self.scene[end - 1]:
            end += 1
        return self.take(end - self.cursor)

    def tags_for(self, source, n):
        t0 = self.clock.get(source, 0)
        self.clock[source] = t0 + n
        return np.array([make_tag(source, (t0 + i) * MS) for i in range(n)], np.int64)

    def register(self, rows):
        """Provenances for ``rows``: their indices in ``src``."""
        first = len(self.src)
        self.src.extend(np.array(r) for r in rows)
        return np.arange(first, first + len(rows), dtype=np.int64)

    def ids_for(self, idx):
        self.seq += 1
        return [f"s{self.seq}_p{int(i)}" for i in idx]

    def live_n(self, total):
        return min(total, self.model.capacity) if self.model.ring else total

    # -- mutators
    def append(self, idx, source, keys=None, rows=None):
        """Keyed, tagged append of pool rows ``idx`` (``rows``: other bits with provenance ``idx``); keys default to
        10,000 + the scene index: the caller's own, never -1 - row id."""
        idx = np.asarray(idx, np.int64)
        rows = self.bits[idx] if rows is None else rows
        keys = 10_000 + self.scene[idx] if keys is None else np.asarray(keys, np.int64)
        tags, ids = self.tags_for(source, idx.size), self.ids_for(idx)
        before = self.model.total
        want = self.model.append(rows, tags, keys, ids, self.register(rows))
        got = self.mem.append(self.io.t(rows), ids=ids, meta=[{"i": i} for i in ids], group=self.io.i64(keys),
                              tag=self.io.i64(tags))
        assert got == want == before, f"append returned {got}, want {want}"
        self.stored += idx.size
        self._note_overwritten()
        return want

    def _note_overwritten(self):
        """The newest row the ring has overwritten, for the probes."""
        if self.model.wrapped and self.model.prov[self.model.base - 1] >= 0:
            self.overwritten = int(self.model.prov[self.model.base - 1])

    def append_novel(self, rows, keys, tau, source):
        """Gated append of ``rows`` with ``keys``; the batch is cut by a row while the live count it leaves is a
        multiple of 16."""
        ks, kr = self.model.known(rows)
        while True:
            keep, _ = N.gate(rows, tau, self.dtype, self.model.total, ks, kr)
            if self.live_n(self.model.total + int(keep.sum())) % 16:
                break
            rows, keys, ks, kr = rows[:-1], keys[:-1], ks[:-1], kr[:-1]
        idx = np.arange(rows.shape[0])
        tags, ids = self.tags_for(source, idx.size), self.ids_for(idx)
        before = self.model.total
        pid = self.register(rows)
        keep, row_of = self.model.append_novel(rows, tau, tags, keys, ids, pid, known=(ks, kr))
        got = self.mem.append_novel(self.io.t(rows), tau, ids=ids, meta=[{"i": i} for i in ids],
                                    group=self.io.i64(keys), tag=self.io.i64(tags))
        _same(got.keep, keep, "append_novel keep")
        _same(got.row_of, row_of, "append_novel row_of")
        assert got.kept == int(keep.sum())
        self.gated.append(float(keep.mean()))
        self.stored += int(keep.sum())
        if (~keep).any():
            self.gone = int(pid[np.nonzero(~keep)[0][-1]])
        self._note_overwritten()
        return keep

    def _erased(self, before_prov, out, got):
        assert got.count == out.count, f"erase count {got.count} != {out.count}"
        _same(got.new_row_of, out.new_row_of, "erase new_row_of")
        gone = np.nonzero(out.new_row_of < 0)[0]
        if gone.size:
            self.gone = int(before_prov[gone[-1]])
            after = np.nonzero(out.new_row_of[gone[0]:] >= 0)[0]
            if after.size:                                  # the first survivor behind the first erased row moved
                self.moved = int(before_prov[gone[0] + after[0]])
                self.join = int(out.new_row_of[gone[0] + after[0]])
        return out

    def erase_rows(self, ids):
        prov = self.model.prov.copy()
        return self._erased(prov, self.model.erase_rows(_np(ids)), self.mem.erase(rows=ids))

    def erase_scopes(self, scopes):
        prov = self.model.prov.copy()
        return self._erased(prov, self.model.erase_scopes(scopes), self.mem.erase(scope=scopes))

    def erase_refused(self, **kw):
        """A wrapped ring refuses the erase on the host mirror: VM_ERR_UNSUPPORTED, the model says the same."""
        assert self.model.erase_rows([0]) is None
        try:
            self.mem.erase(**kw)
        except Exception as e:                              # vidmem._lib.VidmemError, or the fake's
            assert getattr(e, "code", None) == VM_ERR_UNSUPPORTED, repr(e)
            return
        raise AssertionError("the erase on a wrapped ring was not refused")

    def regroup(self, from_row=None):
        if from_row is None:
            want = self.model.regroup_whole(THRESHOLD, GAP_MS)
        else:
            want = self.model.regroup_tail(THRESHOLD, GAP_MS, from_row)
        got = self.mem.regroup_events(THRESHOLD, GAP_MS, from_row)
        assert got == want, f"regroup_events(from_row={from_row}) opened {got} events, want {want}"
        return want

    def reset(self):
        self.model.reset()
        self.mem.reset()
        self.join = None

    def restore(self, capacity):
        """snapshot -> restore: -> a Driver on the restored memory that carries on with this one's data and clocks."""
        other = Driver(self.io.restore(self.mem, capacity), self.model.restored(capacity), self.io, self.hooks)
        for name in ("src", "cursor", "clock", "moved", "gone", "overwritten", "join", "seq", "log", "gated"):
            setattr(other, name, getattr(self, name))
        if self.model.base:
            other.join = None
        self.restored.append(other)
        return other

    # -- probes and the checkpoint
    def probes(self) -> Probes:
        lo, live = self.model.window()
        n = live.rows.shape[0]
        spare = self.bits[-6:]                              # never stored: the scripts stop far below the pool's end
        pick = lambda i, fb: self.src[i] if i is not None else fb
        rnd = int(np.random.default_rng(1000 + len(self.log)).integers(0, max(n, 1)))
        q = np.stack([noisy(live.rows[0] if n else spare[0], self.dtype, 1),
                      noisy(live.rows[-1] if n else spare[1], self.dtype, 2),
                      noisy(pick(self.moved, live.rows[n // 3] if n else spare[2]), self.dtype, 3),
                      np.array(pick(self.gone, spare[3])),
                      np.array(pick(self.overwritten, spare[4])),
                      np.array(live.rows[rnd] if n else spare[5])])
        if n:
            a = n // 2
            src = int(live.tags[a]) >> MS_BITS
            window = (int(live.tags[a]), make_tag(src, (int(live.tags[a]) & ((1 << MS_BITS) - 1)) + 150 * MS))
            one = (make_tag(int(live.tags[-1]) >> MS_BITS, 0), make_tag(int(live.tags[-1]) >> MS_BITS, (1 << MS_BITS) - 1))
        else:
            window, one = (make_tag(0, 0), make_tag(0, 150 * MS)), (make_tag(1, 0), make_tag(1, (1 << MS_BITS) - 1))
        empty = (make_tag(7, 5), make_tag(7, 3))
        pool4 = [SCOPE_ALL, one, window, empty]
        scopes = [pool4[i % 4] for i in range(6)]
        j = n // 2 if self.join is None or not 8 <= self.join <= n - 8 else self.join - 8
        c16 = live.rows[j:j + 16] if n >= 16 + j else self.bits[-22:-6]
        c3 = live.rows[n - 3:] if n >= 3 else self.bits[-25:-22]
        clips = [noisy(c16, self.dtype, 4)[None], noisy(c3, self.dtype, 5)[None]]
        range_min = 0.5
        if n:       # from the oracle's scores: the largest 8th-best in-scope score of a query, so no query has above 7 hits
            sc = cref.cosine_matrix(np.ascontiguousarray(q), np.ascontiguousarray(live.rows), dtype=self.dtype)
            eighth = [np.sort(sc[i][S.scope_mask(live.tags, *scopes[i])])[::-1] for i in range(6)]
            range_min = max(float(e[7]) for e in eighth if e.size > 7)
        return Probes(q, scopes, clips, range_min)

    def check(self, label):
        n = self.model.total - self.model.base
        assert n % 16 or n == 0, f"[{label}] {n} live rows: a multiple of 16 leaves no ragged tile"
        p = self.probes()
        exp = self.model.expect(p)
        for hook in self.hooks:
            hook(label, self, p, exp)
        self.log.append((label, checkpoint(self.mem, self.model, p, self.io, exp, label)))


# ---- the two scripts ---------------------------------------------------------------------------------------------------------
TAU = 0.93                     # the novelty threshold: just above the usual score of two rows of one scene


def _odd(d: Driver, n):
    """A row count near ``n`` that leaves a live count that is no multiple of 16."""
    while d.live_n(d.model.total + n) % 16 == 0:
        n += 1
    return n


def _scenes(d: Driver, n):
    idx = d.take_scenes(n)
    while d.live_n(d.model.total + idx.size) % 16 == 0:
        idx = np.concatenate([idx, d.take_scenes(1)])
    return idx


def _repeats_and_new(d: Driver, stored_from, n_old, n_new):
    """A gated batch: stored scenes again (noisy copies of live rows from index ``stored_from`` on), then new scenes,
    then stored scenes once more."""
    _, live = d.model.window()
    old, old_keys = live.rows[stored_from:stored_from + n_old], 20_000 + live.ords[stored_from:stored_from + n_old]
    new = d.take_scenes(n_new)
    h = old.shape[0] // 2
    rows = np.concatenate([noisy(old[:h], d.dtype, 21, 0.02), d.bits[new], noisy(old[h:], d.dtype, 22, 0.02)])
    keys = np.concatenate([old_keys[:h], 10_000 + d.scene[new], old_keys[h:]])
    return rows, keys


def linear_script(d: Driver):
    """The linear life: capacity 1,600, grouped and tagged, a checkpoint after every step.  -> the driver it ended
    with, the restored memory's."""
    m = d.model
    # 1. keyed, tagged append of source 0: keys come back every 7 scenes
    idx = _scenes(d, 560)
    d.append(idx, 0, keys=10_000 + d.scene[idx] % 7)
    d.check("1 append source 0")
    # 2. a gated batch that repeats stored scenes
    d.append_novel(*_repeats_and_new(d, 40, 90, 190), TAU, 0)
    d.check("2 append_novel")
    # 3. whole regroup
    d.regroup()
    d.check("3 whole regroup")
    # 4. source 1, then a tail regroup from its first row (bf16: the last row lies outside the certificate's domain)
    idx = _scenes(d, 230)
    first = d.append(idx, 1)
    if d.dtype == "bf16":
        while d.live_n(m.total + 1) % 16 == 0:
            d.append(d.take_scenes(1), 1)
        outside = d.append(d.take(1), 1, rows=outside_row(m.D))
    d.regroup(first)
    d.check("4 append source 1, tail regroup")
    # 5. erase a time window in the middle of source 0, then the whole regroup DESIGN.md 16 asks for
    a, n = 200, 150 + ((m.total - 150) % 16 == 0)
    while m.keys[a] == m.keys[a - 1]:
        a += 1                                               # from an event's first row on: 150 frames
    d.erase_scopes([(int(m.tags[a]), int(m.tags[a + n - 1]))])
    d.check("5 erase scope")
    d.regroup()
    d.check("5 whole regroup")
    # 6. erase the rows of a top-k result as returned, -1 padding included
    q = d.probes().queries
    _, rows = d.mem.topk(d.io.t(q), 12, min_score=0.6)
    ids = _np(rows).astype(np.int64)
    assert (ids == -1).any() and (ids >= 0).any()
    extra = [outside] if d.dtype == "bf16" else []
    spare = 0                                                # rows 0 .. spare - 1 too, while the count left is a multiple of 16
    sel = lambda: np.concatenate([ids.ravel(), np.array(extra + list(range(spare)), np.int64)])
    while (m.total - int(E.mask_of_rows(m.total, sel()).sum())) % 16 == 0:
        spare += 1
    d.erase_rows(d.io.i64(sel()))
    d.regroup()
    d.check("6 erase top-k rows, whole regroup")
    # 7. a gated batch again: the vacated, zeroed slots neither suppress nor match, and the new rows reuse them
    d.append_novel(*_repeats_and_new(d, 300, 60, 120), TAU, 2)
    d.check("7 append_novel into vacated slots")
    # 8. snapshot -> restore; the script goes on with the restored memory
    r = d.restore(1600)
    r.check("8 restored")
    d.check("8 original")
    d = r
    m = d.model
    # 9. erase everything; the empty memory; a keyed append whose row ids start at 0 again
    d.erase_scopes([SCOPE_ALL])
    d.check("9 empty")
    idx = _scenes(d, 90)
    assert d.append(idx, 2) == 0
    d.check("9 append after erase-to-empty")
    # 10. reset, then a keyed append whose first key is the last key before the reset: it opens a group
    last = int(m.keys[-1])
    d.reset()
    idx = _scenes(d, 70)
    keys = 10_000 + d.scene[idx]
    keys[keys == keys[0]] = last
    d.append(idx, 0, keys=keys)
    d.check("10 reset, append")
    return d


def ring_script(d: Driver):
    """The ring life: capacity 600, grouped and tagged.  -> the driver it began with."""
    m = d.model
    cap = m.capacity
    # 1. below the capacity; keys come back every 7 scenes (bf16: one row outside the certificate's domain)
    idx = _scenes(d, 200)
    d.append(idx, 0, keys=10_000 + d.scene[idx] % 7)
    if d.dtype == "bf16":
        d.append(d.take(1), 0, rows=outside_row(m.D), keys=[9_999])
    idx = _scenes(d, 350)
    d.append(idx, 0, keys=10_000 + d.scene[idx] % 7)
    d.check("1 append")
    # 2. erase a scope while the ring has not wrapped: six whole scenes, so the scenes before and behind them - one key -
    #    become one group
    starts = np.nonzero(np.concatenate([[True], m.keys[1:] != m.keys[:-1]]))[0]
    g = int(np.searchsorted(starts, 150))
    while True:
        a, b = int(starts[g + 1]), int(starts[g + 7])
        if m.keys[a - 1] == m.keys[b] and (m.total - (b - a) - (d.dtype == "bf16")) % 16:
            break
        g += 1
    scopes = [(int(m.tags[a]), int(m.tags[b - 1]))]
    if d.dtype == "bf16":
        scopes.append((int(m.tags[m.keys == 9_999][0]),) * 2)
    groups_before = int(m.ords[-1]) + 1
    d.erase_scopes(scopes)
    assert int(m.ords[-1]) + 1 == groups_before - 7 - (d.dtype == "bf16")       # six scenes gone, two joined
    d.check("2 erase scope")
    # 3. a gated batch across the first wrap
    d.append_novel(*_repeats_and_new(d, 100, 100, 300), 0.935, 1)
    assert m.wrapped
    d.check("3 append_novel across the wrap")
    # 4. whole regroup in the wrapped ring
    d.regroup()
    d.check("4 whole regroup, wrapped")
    # 5. appends, each followed by a tail regroup; the second wrap falls inside a scene: row 2 x capacity - 1 and row
    #    2 x capacity are one group, in slots capacity - 1 and 0, and the tail regroup that joins them starts in slot 0
    while m.total + 130 < 2 * cap:
        first = d.append(d.take(_odd(d, 110)), 1)
        d.regroup(first)
    n = 2 * cap - m.total
    while d.scene[d.cursor + n] != d.scene[d.cursor + n - 1]:
        d.take(1)                                            # skip pool rows until the cut falls inside a scene
    first = d.append(d.take(n), 1)
    d.regroup(first)
    assert m.total == 2 * cap
    d.check("5 tail regroups up to the second wrap")
    n = 95
    while m.keys[cap + n] == cap + n:
        n += 1                                               # the oldest row left must not be its event's first
    first = d.append(d.take(n), 1)
    assert first == 2 * cap
    d.regroup(first)
    d.check("5 tail regroup from slot 0")
    # 6. erase is refused; the memory is unchanged
    d.erase_refused(rows=[int(m.base) + 3, int(m.base) + 4])
    d.erase_refused(scope=[SCOPE_ALL])
    d.check("6 refused erase")
    # 7. snapshot -> restore into a linear memory
    r = d.restore(cap + 40)
    r.check("7 restored linear")
    # 8. reset, append
    d.reset()
    d.append(_scenes(d, 75), 0)
    d.check("8 reset, append")
    return d
