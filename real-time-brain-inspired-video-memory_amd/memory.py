"""EmbeddingMemory: the HBM-resident replacement for the reference's embedding store.

Reference behaviour mirrored here:
  * append   = ``MERGE (c:Chunk:GraphNode {id}) SET c.embedding = $embedding``  (src/components/neo4j_handler.py:229-242);
               chunks whose embedding is falsy are stored WITHOUT one (:243-253) -> they never enter the search.
  * read-back = ``_get_chunk_embeddings`` (src/components/pre_llm_injector.py:390-412), which re-ships every stored
               vector over bolt for every batch; here rows stay on the device and only (row, score) pairs move.
  * row order = append order (the reference's dict order comes from an unordered Cypher MATCH and is not
               deterministic; the build defines it).

Grouped memories (``grouped=True``) also keep one int64 group key per row: ``topk_grouped`` returns the k best groups
(video chunks), one hit per group, instead of k frames of one moment (include/vidmem.h).

Tagged memories (``tagged=True``) keep one int64 tag per row - which video, and when (``make_tag``) - so that one memory
holds many videos: ``topk_scoped`` ranks only the rows whose tag lies in the query's range (``scope_of``), the
counterpart of the reference's ``{graph_uuid: $graph_uuid}`` predicate (include/vidmem.h).

All arithmetic is in libvidmem.so (csrc/memory.hip, csrc/topk.hip, csrc/topk_exact.hip, csrc/topk_group.hip,
csrc/topk_scope.hip, csrc/novelty.hip, csrc/erase.hip, csrc/range.hip, csrc/events.hip, csrc/summary.hip).

``erase`` forgets rows - a whole video or time window by its tags, or rows by id - and compacts the memory in place, so
that a non-ring memory that has filled up takes new rows again (include/vidmem.h).

``range_search`` returns EVERY row above a threshold, in time order, where the top-k searches return the best k;
``moments`` turns those hits into ``(video, t0, t1, peak)`` runs (csrc/range.hip, include/vidmem.h).

``events`` cuts the stored rows into events - maximal runs of consecutive rows in which each frame resembles the one
before it - and ``regroup_events`` makes those events the groups of ``topk_grouped``: one hit per scene instead of one
per fixed chunk (csrc/events.hip, include/vidmem.h).

``summaries`` turns every group into one centroid row and one key frame, and ``consolidate`` appends those centroids to
a second, small memory that every search runs on unchanged (csrc/summary.hip, include/vidmem.h).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from .scratch import (NOVEL_MAX_ROWS, BiasTopkScratch, ClipScratch, DiverseTopkScratch, EraseScratch, EventsScratch,  # noqa: F401
                      FoldTopkScratch,
                      GroupedScopedTopkScratch, GroupedTopkScratch, MaskedTopkScratch, MixTopkScratch, NoveltyScratch, RangeScratch,
                      ScopedTopkScratch, Scratch, SeqScratch, SpanTopkScratch, SummaryScratch, TopkScratch)


INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
TAG_MS_BITS = 40                 # a tag = source << 40 | milliseconds
TAG_MAX_MS = 1 << TAG_MS_BITS    # ~34.8 years of video per source
TAG_MAX_SOURCE = 1 << 22
SCOPE_ALL = (INT64_MIN, INT64_MAX)  # every row, untagged ones (INT64_MIN) included


def make_tag(source: int, ms: int) -> int:
    """The tag of a row of source (video) ``source`` at ``ms`` milliseconds: ``(source << 40) | ms``, with
    0 <= ms < 2^40 and 0 <= source < 2^22.  Tags of one source are consecutive integers in time order, so one inclusive
    range names a whole source or a time window of it (``scope_of``)."""
    source, ms = int(source), int(ms)
    if not 0 <= source < TAG_MAX_SOURCE:
        raise ValueError(f"source {source} outside [0, 2^22)")
    if not 0 <= ms < TAG_MAX_MS:
        raise ValueError(f"ms {ms} outside [0, 2^40)")
    return (source << TAG_MS_BITS) | ms


def scope_of(source: int, t0_ms: Optional[int] = None, t1_ms: Optional[int] = None) -> Tuple[int, int]:
    """The inclusive tag range ``(lo, hi)`` of source ``source`` between ``t0_ms`` and ``t1_ms`` (both inclusive;
    ``None`` = from its start / to its end).  ``scope_of(3)`` is all of video 3:
    ``(3 << 40, (3 << 40) | (2^40 - 1))``; ``scope_of(3, 180_000, 300_000)`` is video 3 between 180 s and 300 s.
    ``t0_ms > t1_ms`` is a valid, empty scope."""
    lo = make_tag(source, 0 if t0_ms is None else t0_ms)
    hi = make_tag(source, TAG_MAX_MS - 1 if t1_ms is None else t1_ms)
    return lo, hi


class Novelty(NamedTuple):
    """What ``append_novel`` decided: ``keep`` bool [B] and ``row_of`` int64 [B] on the device (the row that stands for
    each frame: its own new id when kept, the row that suppressed it otherwise), ``kept`` the number of stored rows."""
    keep: torch.Tensor
    row_of: torch.Tensor
    kept: int


class Erased(NamedTuple):
    """What ``erase`` did: ``count`` rows are gone; ``new_row_of`` int64 [rows before the call] on the device maps every
    old row id to its new one, -1 for an erased row."""
    count: int
    new_row_of: torch.Tensor


class RangeHits(NamedTuple):
    """What ``enqueue_range`` returns, all on the device: ``counts`` int64 [Q] (the TOTAL hits of each query, also above
    ``max_hits``), ``rows`` int64 [Q, max_hits] (-1 padded) and ``scores`` float64 [Q, max_hits] (0.0 padded)."""
    counts: torch.Tensor
    rows: torch.Tensor
    scores: torch.Tensor


class RangeResult(NamedTuple):
    """One query's entry of ``range_search``: ``rows`` int64 and ``scores`` float64, trimmed to the hits that were
    written, in ascending row id; ``count`` the query's total number of hits (``> len(rows)`` = cut by ``max_hits``)."""
    rows: torch.Tensor
    scores: torch.Tensor
    count: int


class Moment(NamedTuple):
    """A run of hits of one source, close in time (``segment_moments``)."""
    source: int
    t0_ms: int
    t1_ms: int
    first_row: int
    last_row: int
    hits: int
    peak_row: int
    peak_score: float


def segment_moments(rows, scores, tags, max_gap_ms) -> List[Moment]:
    """One query's hits -> moments.  ``rows`` int64 [n] ascending, ``scores`` float64 [n], ``tags`` int64 [n] (the tag
    of each hit row, ``make_tag``'s split: source = tag >> 40, milliseconds = the low 40 bits): numpy in, a list out.

    Walks the hits in row order.  A run continues while the source stays the same and the milliseconds do not decrease
    and grow by at most ``max_gap_ms``; anything else opens a new run.  Hits tagged INT64_MIN have no time and are left
    out.  A run's peak is its highest score, the lowest row on ties.  Moments come back ordered by
    (peak_score descending, first_row ascending), the order relation of every search here."""
    import numpy as np
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    tags = np.asarray(tags, dtype=np.int64).reshape(-1)
    if not (rows.shape == scores.shape == tags.shape):
        raise ValueError("rows, scores and tags differ in length")
    gap = int(max_gap_ms)
    if gap < 0:
        raise ValueError("max_gap_ms is negative")
    timed = tags != INT64_MIN
    rows, scores, tags = rows[timed], scores[timed], tags[timed]
    if rows.size == 0:
        return []
    src = tags >> TAG_MS_BITS
    ms = tags & (TAG_MAX_MS - 1)
    step = ms[1:] - ms[:-1]
    cut = (src[1:] != src[:-1]) | (step < 0) | (step > gap)
    starts = np.concatenate([[0], np.nonzero(cut)[0] + 1])
    ends = np.concatenate([starts[1:], [rows.size]])
    out = []
    for a, b in zip(starts.tolist(), ends.tolist()):
        peak = a + int(np.argmax(scores[a:b]))     # argmax keeps the first = lowest row on ties
        out.append(Moment(int(src[a]), int(ms[a]), int(ms[b - 1]), int(rows[a]), int(rows[b - 1]), b - a,
                          int(rows[peak]), float(scores[peak])))
    out.sort(key=lambda m: (-m.peak_score, m.first_row))
    return out


class EventsOut(NamedTuple):
    """What ``enqueue_events`` returns, all on the device: ``count`` int64 [1] (the TOTAL number of events, also above
    ``max_events``), ``first_rows`` int64 [max_events] (-1 padded), ``event_of`` int64 [capacity] (entries at and beyond
    the live row count are not written) and ``links`` float64 [capacity] or ``None``."""
    count: torch.Tensor
    first_rows: torch.Tensor
    event_of: torch.Tensor
    links: Optional[torch.Tensor]


class Events(NamedTuple):
    """What ``events`` returns: ``first_rows`` int64 (the first row id of every event that was written, ascending),
    ``event_of`` int64 [live rows] (the event index of each live row, oldest first), ``count`` the total number of
    events (``> len(first_rows)`` = cut by ``max_events``) and ``links`` float64 [live rows] or ``None``."""
    first_rows: torch.Tensor
    event_of: torch.Tensor
    count: int
    links: Optional[torch.Tensor]


class Event(NamedTuple):
    """A run of consecutive rows that resemble each other (``segment_events``)."""
    source: Optional[int]
    t0_ms: Optional[int]
    t1_ms: Optional[int]
    first_row: int
    last_row: int
    rows: int


class SummariesOut(NamedTuple):
    """What ``enqueue_summaries`` returns, all on the device, one entry per window slot: ``count`` int64 [1] (the TOTAL
    number of live groups), ``first_rows`` / ``n_rows`` / ``keys`` int64 [max_groups] (-1 padded), ``centroids``
    [max_groups, D] of the memory's dtype (zero-padded), and with key frames ``key_rows`` int64 (-1 padded) and
    ``key_scores`` float64 (0.0 padded), else ``None``."""
    count: torch.Tensor
    first_rows: torch.Tensor
    n_rows: torch.Tensor
    keys: torch.Tensor
    centroids: torch.Tensor
    key_rows: Optional[torch.Tensor]
    key_scores: Optional[torch.Tensor]


class Summaries(NamedTuple):
    """What ``summaries`` returns, trimmed to the groups that were written: per group its first row id, row count,
    group key, centroid row, key frame (the stored row closest to the centroid) and that row's RAW cosine against the
    centroid; ``count`` the total number of live groups."""
    first_rows: torch.Tensor
    n_rows: torch.Tensor
    keys: torch.Tensor
    centroids: torch.Tensor
    key_rows: torch.Tensor
    key_scores: torch.Tensor
    count: int


def segment_events(first_rows, n_rows, base=0, tags=None) -> List[Event]:
    """The events of a memory as a list, in row order.  ``first_rows`` int64 [E] ascending: the first row id of every
    event (``events(...).first_rows``, complete); the live rows are the ids ``base .. base + n_rows - 1``; ``tags`` int64
    [n_rows] or ``None``: the tag of each live row in row order (``tags_host()``; ``make_tag``'s split: source =
    tag >> 40, milliseconds = the low 40 bits).  Event e runs from its first row to the row before the next event's
    first.  ``source`` and ``t0_ms`` come from its first row's tag, ``t1_ms`` from its last row's; an untagged memory or
    rows tagged INT64_MIN give ``None`` for all three (an event never mixes timed and untimed rows, nor two sources)."""
    import numpy as np
    first = np.asarray(first_rows, dtype=np.int64).reshape(-1)
    n_rows, base = int(n_rows), int(base)
    if n_rows < 0:
        raise ValueError("n_rows is negative")
    if first.size == 0:
        if n_rows:
            raise ValueError("live rows but no event: first_rows is incomplete")
        return []
    if first[0] != base or (np.diff(first) <= 0).any() or first[-1] >= base + n_rows:
        raise ValueError("first_rows must start at base, ascend strictly and stay below base + n_rows")
    if tags is not None:
        tags = np.asarray(tags, dtype=np.int64).reshape(-1)
        if tags.size != n_rows:
            raise ValueError(f"{tags.size} tags for {n_rows} rows")
    last = np.concatenate([first[1:] - 1, [base + n_rows - 1]])
    out = []
    for a, b in zip(first.tolist(), last.tolist()):
        source = t0 = t1 = None
        if tags is not None:
            ta, tb = int(tags[a - base]), int(tags[b - base])
            if ta != INT64_MIN and tb != INT64_MIN:
                source, t0, t1 = ta >> TAG_MS_BITS, ta & (TAG_MAX_MS - 1), tb & (TAG_MAX_MS - 1)
        out.append(Event(source, t0, t1, a, b, b - a + 1))
    return out


def _check_erase_selectors(rows, scope) -> None:
    """``erase`` / ``enqueue_erase`` take exactly one selector."""
    if rows is not None and scope is not None:
        raise ValueError("erase takes rows or scope, not both")
    if rows is None and scope is None:
        raise ValueError("erase needs a selector: rows=... or scope=...")


def _torch_dtype(name: str):
    return {"f16": torch.float16, "bf16": torch.bfloat16}[name]


def _ptr(x: Optional[torch.Tensor]) -> C.c_void_p:
    """The address of a tensor for the library; the null pointer for ``None`` and for an empty tensor."""
    return C.c_void_p(x.data_ptr() if x is not None and x.numel() else 0)


def _min_score_args(min_score: Optional[float]) -> Tuple[int, float]:
    """-> (use_min, min_score) as the searches take the optional strict ``> min_score`` filter."""
    return (0, 0.0) if min_score is None else (1, float(min_score))


def _keep_alive(*tensors) -> None:
    """The library reads a call's inputs asynchronously: keep each one (``None`` skipped) until the current stream has
    consumed it."""
    cur = torch.cuda.current_stream()
    for t in tensors:
        if t is not None:
            t.record_stream(cur)


class _Search(NamedTuple):
    """One of the six top-k searches as ``EmbeddingMemory._search`` runs it: its entries, the memory it needs and the
    arguments it takes beyond (queries, k, min_score, score_mode)."""
    words: str                   # the search in an error message
    scratch: type                # its scratch kind (which names the sizing call)
    fast: str                    # the fp32 scan with the exact redo of what it cannot certify
    exact: Optional[str]         # every pair scored exactly
    grouped: bool = False        # needs a grouped memory
    tagged: bool = False         # needs a tagged memory
    refusal: str = ""            # ... and says so in these words
    max_k: int = 64              # 0 = the library's own rule
    scoped: bool = False         # takes a (lo, hi) pair per query: a tag range, or a row-id span
    pairs: str = "scope"         # ... and calls it this in an error message
    masked: bool = False         # takes row masks [n_masks, W] and the mask each query names
    keyed: bool = False          # returns the group keys as a third output
    strided: bool = False        # passes the (row_stride, row_offset) pair
    redo: Optional[str] = None   # a separate second stage that redoes the flagged queries


_PLAIN = _Search("top-k", TopkScratch, "vm_topk_cosine", None, max_k=0, strided=True, redo="vm_topk_redo_flagged")
_GROUPED = _Search("grouped top-k", GroupedTopkScratch, "vm_topk_cosine_grouped", "vm_topk_cosine_grouped_exact",
                   grouped=True, keyed=True,
                   refusal="topk_grouped needs a grouped memory (EmbeddingMemory(..., grouped=True))")
_SCOPED = _Search("scoped top-k", ScopedTopkScratch, "vm_topk_cosine_scoped", "vm_topk_cosine_scoped_exact",
                  tagged=True, scoped=True, strided=True,
                  refusal="topk_scoped needs a tagged memory (EmbeddingMemory(..., tagged=True))")
_MASKED = _Search("masked top-k", MaskedTopkScratch, "vm_topk_cosine_masked", "vm_topk_cosine_masked_exact", masked=True,
                  strided=True)
_SPAN = _Search("span top-k", SpanTopkScratch, "vm_topk_cosine_span", "vm_topk_cosine_span_exact", scoped=True,
                pairs="span", strided=True)
_GROUPED_SCOPED = _Search("scoped grouped top-k", GroupedScopedTopkScratch, "vm_topk_cosine_grouped_scoped",
                          "vm_topk_cosine_grouped_scoped_exact", grouped=True, tagged=True, scoped=True, keyed=True,
                          refusal="topk_grouped_scoped needs a grouped and tagged memory "
                                  "(EmbeddingMemory(..., grouped=True, tagged=True))")


class _Scored(NamedTuple):
    """One of the four searches that rank by a score of their own (mixed, any/all, biased, diverse) as
    ``EmbeddingMemory._scored`` runs it.  Their entries share the middle and the end of the argument list - the masks, the
    ``min_score`` pair, the stride, the outputs, the counter and the flags of the fast entry, the workspace - and differ in
    the operands before it, which each public method normalises itself."""
    words: str                          # the search in an error message
    scratch: type                       # its scratch kind (which names the sizing call)
    fast: str                           # the fp32 scan with the exact redo of what it cannot certify
    exact: str                          # every selected pair scored exactly
    third: Optional[torch.dtype] = None  # a third output [n, k] of this dtype after scores and rows
    scratch_out: Optional[str] = None   # ... or a buffer of the scratch that the library writes there


_MIX = _Scored("mixed top-k", MixTopkScratch, "vm_topk_cosine_mix", "vm_topk_cosine_mix_exact")
_FOLD = _Scored("any/all top-k", FoldTopkScratch, "vm_topk_cosine_fold", "vm_topk_cosine_fold_exact", third=torch.int32)
_BIASED = _Scored("biased top-k", BiasTopkScratch, "vm_topk_cosine_biased", "vm_topk_cosine_biased_exact")
_DIVERSE = _Scored("diverse top-k", DiverseTopkScratch, "vm_topk_cosine_diverse", "vm_topk_cosine_diverse_exact",
                   scratch_out="mmr")


def _last_property(kind: type, name: str, what: str) -> property:
    """``last_*``: a buffer of the scratch that the last call of ``kind`` on this memory used, its own or the caller's."""
    def get(self) -> Optional[torch.Tensor]:
        s = self._last.get(kind)
        return None if s is None else getattr(s, name)
    return property(get, doc=what + " (a device tensor of the scratch that call used; ``None`` before the first call).")


def _count_property(kind: type, what: str) -> property:
    """``*_uncertified_count``: the memory's counter of ``kind``, which counts on whichever scratch a call used."""
    def get(self) -> int:
        c = self._uncert.get(kind)
        return 0 if c is None else int(c.item())
    return property(get, doc=what + " redid exhaustively since this memory was created (one 4-byte read-back; "
                                    "synchronises).")


class EmbeddingMemory:
    def __init__(self, capacity: int, dim: int, dtype: str = "f16", ring: bool = False, device: int = 0,
                 graph_uuid: Optional[str] = None, grouped: bool = False, tagged: bool = False):
        self.ctx = _lib.Context.get(device)
        self.L = self.ctx.L
        self.device = torch.device("cuda", device)
        self.dtype_name = dtype
        self.dtype = _torch_dtype(dtype)
        self.dim = int(dim)
        self.capacity = int(capacity)
        self.ring = bool(ring)
        self.graph_uuid = graph_uuid
        self.grouped = bool(grouped)
        self.tagged = bool(tagged)
        self._next_source = 0       # new_source
        self._next_group_key = 0    # above every key appended from host values (new_group_key)
        self._last_keys_dev = None  # keys of the last grouped append when they were a device tensor (host: unknown)
        self._init_scratch()
        # Host tables: chunk id (reference pre_llm_injector.py:91) and {"time":..., "content":...} (for
        # _vector_search_chunks) of row (table_base + i).  table_base stays 0 unless a ring has wrapped far enough for
        # the slots of overwritten rows to be dropped (see _trim_tables); use id_of / meta_of for row -> entry.
        self.ids: List[Optional[str]] = []
        self.meta: List[Optional[dict]] = []
        self.table_base = 0
        h = C.c_void_p()
        if self.tagged:
            self.ctx.check(self.L.vm_memory_create_tagged(self.ctx.handle, self.capacity, self.dim, _lib.DTYPES[dtype],
                                                          1 if ring else 0, 1 if self.grouped else 0, C.byref(h)))
        else:  # exactly the calls an untagged memory made before tags existed
            create = self.L.vm_memory_create_grouped if self.grouped else self.L.vm_memory_create
            self.ctx.check(create(self.ctx.handle, self.capacity, self.dim, _lib.DTYPES[dtype], 1 if ring else 0,
                                  C.byref(h)))
        self.handle = h

    # ---- scratch: one owner rule for every kind (scratch.py) -----------------------------------------
    def _init_scratch(self) -> None:
        self._own = {}              # scratch kind -> this memory's own instance, made on first use, replaced to grow
        self._last = {}             # scratch kind -> the scratch of the last call of that kind (last_*)
        self._uncert = {}           # scratch kind -> device int32 [1]: what its fast path could not certify (accumulates)

    def _resolve(self, kind: type, scratch: Optional[Scratch], *shape) -> Scratch:
        """The scratch a call of ``shape`` uses.  ``scratch=None``: this memory's own of that kind, created on first use
        and REPLACED by a new object when it does not fit (never resized: a captured graph may hold its addresses).  A
        caller-owned one must fit."""
        if scratch is None:
            scratch = self._own.get(kind)
            if scratch is None:
                scratch = self._own[kind] = kind.for_(self, *shape)
            elif not scratch.fits(self, *shape):
                scratch = self._own[kind] = scratch.grown(self, *shape)     # sized for this call: it fits
        elif not scratch.fits(self, *shape):
            raise ValueError(f"caller-owned {kind.__name__} is too small for this call {shape}")
        return scratch

    def _counter(self, kind: type) -> torch.Tensor:
        """The uncertified counter of a kind: the memory's, whichever scratch a call uses."""
        c = self._uncert.get(kind)
        if c is None:
            c = self._uncert[kind] = torch.zeros(1, dtype=torch.int32, device=self.device)
        return c

    def close(self):
        if getattr(self, "handle", None):
            self.L.vm_memory_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return int(self.L.vm_memory_size(self.handle))

    @property
    def searchable(self) -> int:
        return min(len(self), self.capacity)

    def _as_rows(self, rows) -> torch.Tensor:
        """Accept a device/host tensor or a list of float lists; return a contiguous device tensor in the
        memory dtype (this is the quantisation point: the oracle is evaluated on these 16-bit values)."""
        if not isinstance(rows, torch.Tensor):
            rows = torch.tensor(rows, dtype=torch.float32)
        if rows.dim() == 1:
            rows = rows.unsqueeze(0)
        if rows.shape[-1] != self.dim:
            raise ValueError(f"embedding dimension {rows.shape[-1]} != memory dimension {self.dim}")
        return rows.to(device=self.device, dtype=self.dtype).contiguous()

    def append(self, rows, ids: Optional[Sequence[str]] = None, meta: Optional[Sequence[dict]] = None,
               group=None, tag=None) -> int:
        """Append rows; return the id of the first.  Grouped memories: ``group`` is one key for every row, or one key
        per row (a sequence or an int64 tensor); omitted = this call is one new group (``new_group_key``, never equal to
        the previous call's last key).  A group is a run of consecutive rows with equal keys, so a call whose first key
        equals the previous call's last key continues that group.  A group is searched fast while a query's candidate
        groups hold at most 4,096 rows together (k = 10: about 220 rows per group); larger groups, such as a whole video
        appended in one call, are answered by the exhaustive search every time (exact, slower: DESIGN.md 11).

        Tagged memories: ``tag`` is one int for every row, or one per row (a sequence or an int64 tensor; a device
        tensor is passed through without a host read); omitted = the rows carry INT64_MIN, which only a scope that
        starts at INT64_MIN matches."""
        t = self._as_rows(rows)
        B = t.shape[0]
        if ids is not None and len(ids) != B:
            raise ValueError("ids and rows differ in length")
        keys = self._group_keys_for(B, group)
        tags = self._tags_for(B, tag)
        first, st = C.c_int64(0), _lib.current_stream_ptr()
        if tags is not None:
            rc = self.L.vm_memory_append_tagged(self.handle, _ptr(t), B, _ptr(tags), _ptr(keys), C.byref(first), st)
        elif keys is None:
            rc = self.L.vm_memory_append(self.handle, _ptr(t), B, C.byref(first), st)
        else:
            rc = self.L.vm_memory_append_grouped(self.handle, _ptr(t), B, _ptr(keys), C.byref(first), st)
        self.ctx.check(rc)
        _keep_alive(t, tags, keys)
        self.ids.extend(list(ids) if ids is not None else [None] * B)
        self.meta.extend(list(meta) if meta is not None else [None] * B)
        self._trim_tables()
        return int(first.value)

    # ---- novelty-gated append (include/vidmem.h vm_memory_append_novel) -----------------------------
    def prepare_append_novel(self, B: int) -> "NoveltyScratch":
        """Size this memory's own gated-append buffers for batches of up to ``B`` rows now (before a graph capture: a
        capture must not allocate)."""
        return self._resolve(NoveltyScratch, None, int(B))

    @staticmethod
    def _check_threshold(threshold) -> float:
        tau = float(threshold)
        if math.isnan(tau):
            raise ValueError("the novelty threshold is NaN")
        return tau

    def _known_pair(self, known, B: int):
        """``known=(scores, rows)``, each [B] or [B, k] -> (scores, rows, stride): device float64 / int64 tensors whose
        element i * stride is row i's best score / the row that reached it (column 0 of a top-k result, in place)."""
        if not isinstance(known, (tuple, list)) or len(known) != 2:
            raise ValueError("known must be a pair (scores, rows)")
        ks, kr = known
        if not isinstance(ks, torch.Tensor) or not isinstance(kr, torch.Tensor):
            raise ValueError("known scores and rows must be tensors")
        if ks.dim() not in (1, 2) or kr.shape != ks.shape:
            raise ValueError("known scores and rows must both be [B] or [B, k]")
        if ks.shape[0] != B:
            raise ValueError(f"known results for {ks.shape[0]} rows, batch of {B}")
        if ks.dim() == 2:
            if ks.shape[1] < 1:
                raise ValueError("known results with k = 0")
            ks, kr = ks[:, 0], kr[:, 0]
        ks = ks.to(device=self.device, dtype=torch.float64)
        kr = kr.to(device=self.device, dtype=torch.int64)
        if B > 1 and (ks.stride(0) != kr.stride(0) or ks.stride(0) < 1):
            ks, kr = ks.contiguous(), kr.contiguous()
        return ks, kr, (int(ks.stride(0)) if B > 1 else 1)

    def enqueue_append_novel(self, rows, threshold, known=None, group=None, tag=None,
                             scratch: Optional["NoveltyScratch"] = None
                             ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The capturable gated append -> (keep int32 [B] 0 / 1, row_of int64 [B], count int32 [1]): views of the
        buffers of ``scratch`` (default: this memory's own, ``prepare_append_novel``), valid until the next call on it.

        Enqueues ``vm_memory_append_novel`` on the current stream: nothing is read on the host, the id / meta tables and
        the host row count are not touched - ``sync()`` afterwards brings them in line (rows get ``None`` entries, as
        after replays of ``append``).  ``known=(scores, rows)``: ``[B]`` or ``[B, k]`` tensors of a search the caller
        already ran (RAW scores, no ``min_score``); ``None`` = the gate is among the batch only.  At most 4,096 rows.
        Inside a graph capture pass ``group`` / ``tag`` as device tensors (rewritten in place between replays) and a
        ``scratch`` the session owns."""
        tau = self._check_threshold(threshold)
        t = self._as_rows(rows)
        B = t.shape[0]
        if B > NOVEL_MAX_ROWS:
            raise ValueError(f"a gated append takes at most {NOVEL_MAX_ROWS} rows per call, got {B}")
        ks = kr = None
        stride = 1
        if known is not None:
            ks, kr, stride = self._known_pair(known, B)
        keys = self._group_keys_for(B, group)
        tags = self._tags_for(B, tag)
        return self._append_novel_call(t, tau, ks, kr, stride, keys, tags, scratch)

    def _append_novel_call(self, t, tau, ks, kr, stride, keys, tags, scratch):
        B = t.shape[0]
        scratch = self._resolve(NoveltyScratch, scratch, B)
        self.ctx.check(self.L.vm_memory_append_novel(
            self.handle, _ptr(t), B, tau, _ptr(ks), _ptr(kr), int(stride), _ptr(tags), _ptr(keys), _ptr(scratch.keep),
            _ptr(scratch.row_of), _ptr(scratch.count), _ptr(scratch.ws), scratch.ws.numel(), _lib.current_stream_ptr()))
        _keep_alive(t, ks, kr, keys, tags)
        return scratch.keep[:B], scratch.row_of[:B], scratch.count

    def append_novel(self, rows, threshold, against="memory", known=None, ids: Optional[Sequence[str]] = None,
                     meta: Optional[Sequence[dict]] = None, group=None, tag=None) -> Novelty:
        """Append only the rows that nothing resembles -> ``Novelty(keep, row_of, kept)``.

        In row order a row is dropped when a stored row scores above ``threshold`` against it (``against``), or an
        earlier KEPT row of the batch does; a score equal to the threshold keeps the row.  Scores are the reference
        cosine of ``topk``, bit for bit, so this equals the one-row-at-a-time loop "search, append iff the best score
        is not above the threshold" (include/vidmem.h vm_memory_append_novel).

        ``against``: ``"memory"`` (default) = ``topk(rows, 1)`` over everything stored, redo included (skipped on an
        empty memory); a scope ``(lo, hi)`` / Q pairs / int64 ``[B, 2]`` tensor on a tagged memory =
        ``topk_scoped(rows, 1, scope)`` ("new for this video", "new within the last minute"); ``None`` = among the
        batch only.  ``known=(scores, rows)``: ``[B]`` or ``[B, k]`` tensors of a search the caller already ran, used
        INSTEAD of ``against`` - they must be RAW scores of a search without ``min_score``: a mapped or filtered score
        would be compared with the threshold as if it were the cosine.
        ``ids`` / ``meta``: one entry per row of the batch; only the kept rows' entries are recorded.  ``group`` /
        ``tag``: as in ``append``, per row of the batch; ``group=None`` on a grouped memory = the kept rows of this
        call are one new group.

        This form SYNCHRONISES once per call: it reads ``keep`` back to extend the id / meta tables and brings the row
        count in line (``enqueue_append_novel`` is the form that does not).  Batches above 4,096 rows are walked in
        slices of 4,096, each slice searched after the previous one was appended; with ``known`` or ``against=None``
        such a batch is refused (later slices would not be compared with the earlier ones)."""
        tau = self._check_threshold(threshold)
        whole = isinstance(against, str) and against == "memory"
        if known is not None and not whole:
            raise ValueError("known replaces the search: give known or against, not both")
        scope = None
        if known is None and against is not None and not whole:
            if isinstance(against, str):
                raise ValueError(f"against must be 'memory', a scope or None, got {against!r}")
            if not self.tagged:
                raise ValueError("a scope needs a tagged memory (EmbeddingMemory(..., tagged=True))")
            scope = against
        t = self._as_rows(rows)
        B = t.shape[0]
        if ids is not None and len(ids) != B:
            raise ValueError("ids and rows differ in length")
        if meta is not None and len(meta) != B:
            raise ValueError("meta and rows differ in length")
        ks = kr = None
        stride = 1
        if known is not None:
            ks, kr, stride = self._known_pair(known, B)
        if B > NOVEL_MAX_ROWS and (known is not None or against is None):
            raise ValueError(f"more than {NOVEL_MAX_ROWS} rows need against='memory' or a scope")
        sc = self._scopes(scope, B).t() if scope is not None else None     # [B, 2] view
        keys = self._group_keys_for(B, group)
        tags = self._tags_for(B, tag)
        keep_parts, row_parts, kept = [], [], 0
        for lo in range(0, B, NOVEL_MAX_ROWS):
            hi = min(B, lo + NOVEL_MAX_ROWS)
            part = t[lo:hi]
            s_ks, s_kr, s_stride = ks, kr, stride
            if known is None and against is not None and self.searchable:
                if scope is None:
                    s_ks, s_kr = self.topk(part, 1)
                else:
                    s_ks, s_kr = self.topk_scoped(part, 1, sc[lo:hi].contiguous())
                s_ks, s_kr, s_stride = s_ks[:, 0], s_kr[:, 0], 1
            keep_i, row_of, _ = self._append_novel_call(part, tau, s_ks, s_kr, s_stride,
                                                        None if keys is None else keys[lo:hi],
                                                        None if tags is None else tags[lo:hi], None)
            keep = keep_i.ne(0)
            row_of = row_of.clone()
            picks = torch.nonzero(keep).flatten().tolist()      # the one synchronising read
            self.ids.extend([ids[lo + i] for i in picks] if ids is not None else [None] * len(picks))
            self.meta.extend([meta[lo + i] for i in picks] if meta is not None else [None] * len(picks))
            self.sync()
            keep_parts.append(keep)
            row_parts.append(row_of)
            kept += len(picks)
        if not keep_parts:
            return Novelty(torch.zeros(0, dtype=torch.bool, device=self.device),
                           torch.zeros(0, dtype=torch.int64, device=self.device), 0)
        if len(keep_parts) == 1:
            return Novelty(keep_parts[0], row_parts[0], kept)
        return Novelty(torch.cat(keep_parts), torch.cat(row_parts), kept)

    # ---- erase (include/vidmem.h vm_memory_erase_scoped / vm_memory_erase_rows) ----------------------
    def prepare_erase(self, segment_rows: int = 0) -> "EraseScratch":
        """Size this memory's own erase buffers now (before a graph capture: a capture must not allocate).
        ``segment_rows``: rows that move through the scratch at a time; 0 = the library's default."""
        return self._resolve(EraseScratch, None, int(segment_rows))

    def enqueue_erase(self, rows=None, scope=None, scratch: Optional["EraseScratch"] = None
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
        """The capturable erase -> (new_row_of int64 [capacity], erased int64 [1]): the buffers of ``scratch`` (default:
        this memory's own, ``prepare_erase``), valid until the next call on it.  Entries of ``new_row_of`` at and beyond
        the row count before the call are not written.

        Enqueues ``vm_memory_erase_rows`` / ``vm_memory_erase_scoped`` on the current stream: nothing is read on the
        host, the id / meta tables and the host row count are not touched - ``sync()`` afterwards brings the count in
        line (the tables are then cut to it, not remapped: ``erase`` is the form that remaps them).  Inside a graph
        capture pass ``scope`` as an int64 ``[n, 2]`` device tensor or ``rows`` as an int64 device tensor (rewritten in
        place between replays) and a ``scratch`` the session owns."""
        _check_erase_selectors(rows, scope)
        if scope is not None and not self.tagged:
            raise ValueError("erase by scope needs a tagged memory (EmbeddingMemory(..., tagged=True))")
        scratch = self._resolve(EraseScratch, scratch)     # any segment size serves: prepare_erase chooses one
        tail = (_ptr(scratch.new_row_of), _ptr(scratch.erased), _ptr(scratch.ws), scratch.ws.numel(),
                _lib.current_stream_ptr())
        if scope is not None:
            sel = self._scopes(scope)
            self.ctx.check(self.L.vm_memory_erase_scoped(self.handle, _ptr(sel[0]), _ptr(sel[1]), sel.shape[1], *tail))
        else:
            if isinstance(rows, torch.Tensor):
                sel = rows.to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
            else:
                sel = torch.tensor([int(r) for r in rows], dtype=torch.int64).to(self.device)
            self.ctx.check(self.L.vm_memory_erase_rows(self.handle, _ptr(sel), sel.numel(), *tail))
        _keep_alive(sel)
        return scratch.new_row_of, scratch.erased

    def erase(self, rows=None, scope=None) -> Erased:
        """Forget rows and close the gaps -> ``Erased(count, new_row_of)``.

        Exactly one selector: ``scope`` = one inclusive tag range ``(lo, hi)`` (``scope_of(3)``: all of video 3) or a
        sequence of them, on a tagged memory - a row goes when its tag lies in at least one; ``rows`` = a sequence or
        tensor of row ids, any shape - ids below 0 or beyond the end are ignored and duplicates are allowed, so the
        ``rows`` of a top-k result are passed as they are.
        The survivors keep their order and are renumbered 0 .. n'-1; everything the memory holds - rows, norms, tags,
        group keys, groups - is then what a fresh memory would hold after one append of the survivors (two groups with
        one key that become adjacent are one group), and the freed capacity takes new rows.  The id / meta tables are
        remapped (``id_of(new) ==`` the old id) and ``len()`` follows.  Keys of rows that were appended without a
        group keep their value (include/vidmem.h).
        A ring that has wrapped is refused.  This form SYNCHRONISES once (``enqueue_erase`` is the form that does not)."""
        _check_erase_selectors(rows, scope)
        new_row_of, erased = self.enqueue_erase(rows=rows, scope=scope)
        total = int(self.L.vm_memory_sync(self.handle, _lib.current_stream_ptr()))     # the one wait
        if total < 0:
            self.ctx.check(total)
        count = int(erased.item())
        if count < 0:
            raise _lib.VidmemError(_lib.VM_ERR_UNSUPPORTED, "erase: the ring has wrapped (the host row count was stale)")
        n_old = total + count
        out = new_row_of[:n_old].clone() if count else torch.arange(n_old, dtype=torch.int64, device=self.device)
        if count:
            kept = torch.nonzero(out >= 0).flatten().tolist()
            pad = [None] * max(0, n_old - self.table_base - len(self.ids))
            ids, meta = self.ids + pad, self.meta + pad
            self.ids = [ids[i - self.table_base] for i in kept]
            self.meta = [meta[i - self.table_base] for i in kept]
            self.table_base = 0
        self.sync()
        if self.grouped:   # what a later append(group=None) must not repeat: the last survivor's key (read only then)
            keys = _tensor_from_ptr(self.L.vm_memory_group_keys(self.handle), (max(total, 1),), torch.int64, self.device)
            self._last_keys_dev = keys[total - 1:total].clone() if total else None
        return Erased(count, out)

    def new_source(self) -> int:
        """A source index no earlier ``new_source`` call of this memory returned: one per video (``make_tag``)."""
        src = self._next_source
        self._next_source += 1
        return src

    def _int64_column(self, value, B: int, what: str) -> Tuple[torch.Tensor, Optional[List[int]]]:
        """One int for every row, one per row as a sequence, or an int64 tensor (a 0-dim one counts as one int; any other
        is passed to the device without a host read) -> (device int64 [B], the values where the host knows them)."""
        known = None
        if isinstance(value, torch.Tensor) and value.dim() > 0:
            col = value.to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        elif isinstance(value, (list, tuple)) or (hasattr(value, "shape") and len(value.shape) > 0):
            known = [int(x) for x in value]
            col = torch.tensor(known, dtype=torch.int64).to(self.device)
        else:
            known = [int(value)]
            col = torch.full((B,), known[0], dtype=torch.int64, device=self.device)
        if col.numel() != B:
            raise ValueError(f"{col.numel()} {what} for {B} rows")
        return col, known

    def _int64_cell(self, value) -> torch.Tensor:
        """An int, or a device tensor whose first element counts (not read on the host) -> device int64 [1]."""
        if isinstance(value, torch.Tensor):
            return value.to(device=self.device, dtype=torch.int64).reshape(-1)[:1].contiguous()
        return torch.tensor([int(value)], dtype=torch.int64).to(self.device)

    def _tags_for(self, B: int, tag) -> Optional[torch.Tensor]:
        if tag is None:
            return None
        if not self.tagged:
            raise ValueError("tags need a tagged memory (EmbeddingMemory(..., tagged=True))")
        return self._int64_column(tag, B, "tags")[0]

    def new_group_key(self) -> int:
        """A key no earlier ``new_group_key`` call of this memory returned (and above every key appended so far from
        host values): two videos in one memory never merge their chunk 0."""
        key = self._next_group_key
        self._next_group_key += 1
        return key

    def _group_keys_for(self, B: int, group) -> Optional[torch.Tensor]:
        if not self.grouped:
            if group is not None:
                raise ValueError("group keys need a grouped memory (EmbeddingMemory(..., grouped=True))")
            return None
        if group is None:
            # one NEW group: the key must differ from the previous call's last key, or the device would continue that
            # group.  Host-given keys already raised the counter above it; device-given ones are read back here (one
            # synchronising read - pass `group` explicitly inside a graph capture)
            if self._last_keys_dev is not None and self._last_keys_dev.numel():
                self._next_group_key = max(self._next_group_key, int(self._last_keys_dev[-1]) + 1)
            group = self.new_group_key()
        keys, known = self._int64_column(group, B, "group keys")
        self._last_keys_dev = keys if known is None else None
        if known:
            self._next_group_key = max(self._next_group_key, max(known) + 1)
        return keys

    def _trim_tables(self) -> None:
        """A rolling window must not keep one table slot per row EVER appended: once a ring holds more than two
        capacities (+1024) of slots, those of rows that have been overwritten are dropped."""
        if self.ring and len(self.ids) > 2 * self.capacity + 1024:
            drop = len(self.ids) - self.capacity
            del self.ids[:drop], self.meta[:drop]
            self.table_base += drop

    def sync(self) -> int:
        """Bring the host mirror (row count, id / meta tables) in line with the device counter: call after hipGraph
        replays (streaming.StreamingSession) before eager appends, exhaustive searches or snapshots.  Rows appended
        by replays get ``None`` ids; a captured-but-never-run append is dropped."""
        total = int(self.L.vm_memory_sync(self.handle, _lib.current_stream_ptr()))
        if total < 0:
            self.ctx.check(total)
        n = max(0, total - self.table_base)
        del self.ids[n:], self.meta[n:]
        self.ids.extend([None] * (n - len(self.ids)))
        self.meta.extend([None] * (n - len(self.meta)))
        self._trim_tables()
        return total

    def prepare_topk(self, Q: int, k: int) -> TopkScratch:
        """Size the shared top-k scratch for (Q, k) now, so a later eager call allocates nothing."""
        return self._resolve(TopkScratch, None, int(Q), int(k))

    def reset(self):
        self.ctx.check(self.L.vm_memory_reset(self.handle, _lib.current_stream_ptr()))
        self._next_group_key = 0
        self._next_source = 0
        self._last_keys_dev = None
        self.ids.clear()
        self.meta.clear()
        self.table_base = 0

    def rows_tensor(self) -> torch.Tensor:
        """Zero-copy view of the searchable physical rows [min(size, capacity), D] (debug / snapshot)."""
        n = self.searchable
        ptr = self.L.vm_memory_rows(self.handle)
        return _tensor_from_ptr(ptr, (n, self.dim), self.dtype, self.device)

    # ------------------------------------------------------------------------------------------------------
    def topk(self, queries, k: int, min_score: Optional[float] = None, score_mode: int = _lib.VM_SCORE_RAW,
             row_stride: int = 1, row_offset: int = 0, exact: bool = False, redo: bool = True,
             scratch: Optional["TopkScratch"] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (scores [Q,k] float64, rows [Q,k] int64, -1 padded), ordered (score desc, row asc): ALWAYS the
        exhaustive answer, as the reference returns it (src/components/pre_llm_injector.py:356-370).

        Fast path = fp32 MFMA scan + exact fp64 re-scoring (csrc/topk.hip), which marks the queries it cannot
        certify (more exact ties than candidate slots, gaps below the fp32 bound) in a per-query flag array;
        ``vm_topk_redo_flagged`` (csrc/topk_exact.hip) then redoes exactly those queries exhaustively on the device.
        Both read flags and row count from device memory: no host read-back, graph-capturable.  ``redo=False`` skips
        the second stage (measurement of the scan alone).  k > 58 and ``exact=True`` run the all-query exhaustive
        kernel.  A query of the wrong length scores 0.0 against every row in the reference (:378-379); here it raises
        in ``_as_rows`` unless the caller filters it (similarity.batch_similarities does).

        ``scratch``: workspaces + flag / counter buffers owned by the caller (streaming sessions capture their
        addresses into a hipGraph); default = this memory's own, used by eager calls on the current stream.
        """
        if not exact and k <= 58:
            return self._search(_PLAIN, queries, k, None, min_score, score_mode, False, scratch,
                                (row_stride, row_offset), redo)
        q = self._as_rows(queries)
        Q = q.shape[0]
        scores = torch.empty((Q, k), dtype=torch.float64, device=self.device)
        rows = torch.empty((Q, k), dtype=torch.int64, device=self.device)
        need = int(self.L.vm_topk_exact_workspace_bytes(self.handle, Q, k))
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        self.ctx.check(self.L.vm_topk_cosine_exact(
            self.handle, _ptr(q), Q, k, *_min_score_args(min_score), int(score_mode), int(row_stride),
            int(row_offset), _ptr(scores), _ptr(rows), _ptr(ws), ws.numel(), _lib.current_stream_ptr()))
        _keep_alive(ws)
        return scores, rows

    def _search(self, kind: _Search, queries, k, scope, min_score, score_mode, exact, scratch, stride=(1, 0),
                redo=True) -> Tuple[torch.Tensor, ...]:
        """The one body of ``topk``, ``topk_grouped``, ``topk_scoped``, ``topk_grouped_scoped``, ``topk_span`` (whose
        ``scope`` is the row-id spans) and ``topk_masked`` (whose ``scope`` is the pair (mask, mask_index)).  The memory-kind, ``k`` and mask checks come before anything
        that needs a device."""
        if (kind.grouped and not self.grouped) or (kind.tagged and not self.tagged):
            raise ValueError(kind.refusal)
        if kind.max_k and not 1 <= int(k) <= kind.max_k:
            raise ValueError(f"{kind.words} supports 1 <= k <= {kind.max_k}, got {k}")
        masks = self._masks(scope[0]) if kind.masked else None
        q = self._as_rows(queries)
        Q, k = q.shape[0], int(k)
        sc = self._scopes(scope, Q, kind.pairs) if kind.scoped else None
        if kind.masked:
            sc = self._mask_index(scope[1], masks.shape[0], Q)
        s = self._resolve(kind.scratch, scratch, Q, k)
        outs = [torch.empty((Q, k), dtype=dt, device=self.device)
                for dt in (torch.float64, torch.int64, torch.int64)[:3 if kind.keyed else 2]]
        head = [self.handle, _ptr(q), Q, k]
        if kind.scoped:
            head += [_ptr(sc[0]), _ptr(sc[1])]
        if kind.masked:
            head += [_ptr(masks), masks.shape[0], _ptr(sc)]
        head += [*_min_score_args(min_score), int(score_mode)]
        if kind.strided:
            head += [int(stride[0]), int(stride[1])]
        outp = [_ptr(o) for o in outs]
        st = _lib.current_stream_ptr()
        if exact:
            self.ctx.check(getattr(self.L, kind.exact)(*head, *outp, _ptr(s.ws), s.ws.numel(), st))
        else:   # plain top-k counts on its scratch (a session reads its own), the others on the memory
            uncert = s.uncert if kind is _PLAIN else self._counter(kind.scratch)
            self.ctx.check(getattr(self.L, kind.fast)(*head, *outp, _ptr(uncert), _ptr(s.flags), _ptr(s.ws),
                                                      s.ws.numel(), st))
            if kind.redo and redo:
                self.ctx.check(getattr(self.L, kind.redo)(*head, _ptr(s.flags), *outp, _ptr(s.redo_ws),
                                                          s.redo_ws.numel(), st))
        _keep_alive(q, sc, masks)
        self._last[kind.scratch] = s
        return tuple(outs)

    def _prepare_search(self, kind: _Search, Q: int, k: int) -> Scratch:
        self._counter(kind.scratch)
        return self._resolve(kind.scratch, None, int(Q), int(k))

    def _scored(self, kind: _Scored, k, operands, mask, mask_index, min_score, exact, scratch, stride, first=None,
                sized_by=None) -> Tuple[torch.Tensor, ...]:
        """The one body of ``topk_mix``, ``topk_fold``, ``topk_biased`` and ``topk_diverse``.  ``first`` (optional) runs
        after the ``k`` and ``min_score`` checks and before the mask is looked at; ``operands(what first returned)`` runs
        after the mask checks and returns ``(n, front, keep)``: the number of queries, the entry's arguments between the
        memory and the masks, and the tensors among them to keep alive.  ``sized_by``: what the scratch is sized by in
        place of ``k`` (the diverse search's pool).  Every check comes before anything that needs a device."""
        if not 1 <= int(k) <= 64:
            raise ValueError(f"{kind.words} supports 1 <= k <= 64, got {k}")
        if min_score is not None and math.isnan(float(min_score)):
            raise ValueError("min_score is NaN")
        early = first() if first is not None else None
        masks = self._masks(mask) if mask is not None else None
        if masks is None and mask_index is not None:
            raise ValueError("a mask_index needs a mask")
        n, front, keep = operands(early)
        k = int(k)
        idx = self._mask_index(mask_index, masks.shape[0], n) if masks is not None else None
        s = self._resolve(kind.scratch, scratch, n, k if sized_by is None else sized_by)
        outs = [torch.empty((n, k), dtype=dt, device=self.device)
                for dt in (torch.float64, torch.int64, kind.third) if dt is not None]
        head = [self.handle, *front, _ptr(masks), 0 if masks is None else masks.shape[0], _ptr(idx),
                *_min_score_args(min_score), int(stride[0]), int(stride[1]), *(_ptr(o) for o in outs)]
        if kind.scratch_out:
            head.append(_ptr(getattr(s, kind.scratch_out)))
        tail = (_ptr(s.ws), s.ws.numel(), _lib.current_stream_ptr())
        if exact:
            self.ctx.check(getattr(self.L, kind.exact)(*head, *tail))
        else:
            self.ctx.check(getattr(self.L, kind.fast)(*head, _ptr(self._counter(kind.scratch)), _ptr(s.flags), *tail))
        _keep_alive(*keep, masks, idx)
        self._last[kind.scratch] = s
        return tuple(outs)

    def prepare_topk_grouped(self, Q: int, k: int) -> GroupedTopkScratch:
        """Size the grouped top-k workspace for (Q, k) now (before a graph capture: a capture must not allocate)."""
        return self._prepare_search(_GROUPED, Q, k)

    def topk_grouped(self, queries, k: int, min_score: Optional[float] = None, score_mode: int = _lib.VM_SCORE_RAW,
                     exact: bool = False, scratch: Optional[GroupedTopkScratch] = None
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """-> (scores [Q,k] float64, rows [Q,k] int64, keys [Q,k] int64): the k best GROUPS of a grouped memory.

        The exhaustive row ranking of ``topk`` (score desc, row asc; score mapping and > min_score filter) with only the
        first row of each group kept: a group scores the exact max over its rows, ``rows`` holds the lowest row id
        reaching it, ``keys`` its group key; -1 / 0.0 / -1 padded.  Always the exhaustive answer: the fp32 fast path
        redoes the queries it cannot certify on the device, in the same call (csrc/topk_group.hip).  ``exact=True``
        scores every row exactly for every query (slow).  1 <= k <= 64.  The per-query flags of the last call (why a
        query was redone, vm_topk_flag) are in ``last_group_flags``.  ``scratch``: as in ``topk`` - a
        ``GroupedTopkScratch`` the caller owns (a graph capture), default this memory's own."""
        return self._search(_GROUPED, queries, k, None, min_score, score_mode, exact, scratch)

    def prepare_topk_scoped(self, Q: int, k: int) -> ScopedTopkScratch:
        """Size the scoped top-k workspace for (Q, k) now (before a graph capture: a capture must not allocate)."""
        return self._prepare_search(_SCOPED, Q, k)

    def _scopes(self, scope, n: Optional[int] = None, what: str = "scope") -> torch.Tensor:
        """-> device int64 [2, n] (row 0 = lo, row 1 = hi) from one (lo, hi), a sequence of pairs, or an int64 [n, 2]
        tensor (a device tensor is not read on the host).  ``n`` given: exactly ``n`` pairs, one pair standing for all
        of them; ``n=None``: any number of pairs, at least one.  ``what``: the word for a pair in an error message."""
        if isinstance(scope, torch.Tensor):
            if scope.dtype != torch.int64 or scope.dim() != 2 or scope.shape[1] != 2:
                raise ValueError(f"a {what} tensor must be int64 [n, 2]")
            pairs, count = None, scope.shape[0]
        else:
            pairs = list(scope)
            if len(pairs) == 2 and not hasattr(pairs[0], "__len__"):
                pairs = [pairs] * (1 if n is None else n)
            count = len(pairs)
        if n is None and count < 1:
            raise ValueError(f"0 {what}s: at least one pair (lo, hi) is needed")
        if n is not None and count != n:
            raise ValueError(f"{count} {what}s for {n} queries")
        if pairs is None:
            return scope.to(self.device).t().contiguous()
        if any(len(p) != 2 for p in pairs):
            raise ValueError(f"a {what} is a pair (lo, hi)")
        vals = [[int(p[0]) for p in pairs], [int(p[1]) for p in pairs]]
        return torch.tensor(vals, dtype=torch.int64).to(self.device)

    def topk_scoped(self, queries, k: int, scope, min_score: Optional[float] = None,
                    score_mode: int = _lib.VM_SCORE_RAW, exact: bool = False,
                    scratch: Optional[ScopedTopkScratch] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (scores [Q,k] float64, rows [Q,k] int64): the k best rows of a tagged memory whose tag lies in the query's
        scope, an inclusive range ``(lo, hi)``: one for all queries, a sequence of Q pairs, or an int64 ``[Q, 2]`` tensor
        (``scope_of`` builds the range of a video or of a time window of it).

        The exhaustive row ranking of ``topk`` (score desc, row asc; score mapping and > min_score filter) over the
        in-scope rows only; -1 / 0.0 padded; an empty scope gives an all-padded row.  Always the exhaustive answer: the
        fp32 fast path redoes the queries it cannot certify on the device, in the same call (csrc/topk_scope.hip).
        ``exact=True`` scores every in-scope pair exactly (slow).  1 <= k <= 64.  The per-query flags of the last call
        (why a query was redone, vm_topk_flag) are in ``last_scope_flags``.  ``scratch``: as in ``topk`` - a
        ``ScopedTopkScratch`` the caller owns (a graph capture), default this memory's own."""
        return self._search(_SCOPED, queries, k, scope, min_score, score_mode, exact, scratch)

    def prepare_topk_grouped_scoped(self, Q: int, k: int) -> GroupedScopedTopkScratch:
        """Size the scoped grouped top-k workspace for (Q, k) now (before a graph capture: a capture must not allocate)."""
        return self._prepare_search(_GROUPED_SCOPED, Q, k)

    def topk_grouped_scoped(self, queries, k: int, scope, min_score: Optional[float] = None,
                            score_mode: int = _lib.VM_SCORE_RAW, exact: bool = False,
                            scratch: Optional[GroupedScopedTopkScratch] = None
                            ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """-> (scores [Q,k] float64, rows [Q,k] int64, keys [Q,k] int64): the k best GROUPS of a tagged, grouped memory
        among the rows whose tag lies in the query's scope - one hit per event within a video or a time window.
        ``scope`` is ``topk_scoped``'s: one ``(lo, hi)`` for all queries, a sequence of Q pairs, or an int64 ``[Q, 2]``
        tensor (``scope_of`` builds the range of a video or of a time window of it).

        The exhaustive row ranking of ``topk_scoped`` (in-scope rows only; score desc, row asc; score mapping and
        > min_score filter) with only the first row of each group kept: a group scores the exact max over its IN-SCOPE
        rows, ``rows`` holds the lowest in-scope row id reaching it, ``keys`` its group key; -1 / 0.0 / -1 padded.  Groups
        are the memory's own (runs over all live rows): a window that cuts an event in two neither splits it nor merges
        its neighbours, and a group with no in-scope row is not returned.  Always the exhaustive answer: the fp32 fast
        path redoes the queries it cannot certify on the device, in the same call (csrc/topk_group_scope.hip).
        ``exact=True`` scores every in-scope pair exactly (slow).  1 <= k <= 64.  The per-query flags of the last call
        (why a query was redone, vm_topk_flag) are in ``last_group_scope_flags``.  ``scratch``: as in ``topk`` - a
        ``GroupedScopedTopkScratch`` the caller owns (a graph capture), default this memory's own."""
        return self._search(_GROUPED_SCOPED, queries, k, scope, min_score, score_mode, exact, scratch)

    # ---- row masks and the masked search (include/vidmem.h vm_topk_cosine_masked) -------------------
    @property
    def mask_words(self) -> int:
        """W: the 32-bit words of one row mask of this memory (``vm_memory_mask_words``: the capacity rounded up to 64
        rows, / 32)."""
        return (self.capacity + 63) // 64 * 2

    def new_mask(self, n: int = 1) -> torch.Tensor:
        """-> device int32 ``[n, W]``, all bits clear: ``n`` row masks.  The bit of row id ``r`` is bit ``s & 31`` of word
        ``s >> 5`` with ``s = r % capacity``; bits of slots without a live row are ignored by every consumer, so masks
        combine freely with ``& | ~``.  A mask speaks about ROW IDS: after an erase (which renumbers rows) or a ring
        overwrite it is stale exactly as a stored row id is."""
        return torch.zeros((int(n), self.mask_words), dtype=torch.int32, device=self.device)

    def _masks(self, mask) -> torch.Tensor:
        """-> contiguous device int32 ``[n_masks, W]`` from one mask ``[W]`` or several ``[n_masks, W]``; anything else is
        refused before the library is called."""
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.int32:
            raise ValueError("a mask is an int32 tensor (EmbeddingMemory.new_mask)")
        if mask.dim() not in (1, 2) or mask.shape[0] == 0:
            raise ValueError(f"a mask is [W] or [n_masks, W] with n_masks >= 1, got {tuple(mask.shape)}")
        if mask.shape[-1] != self.mask_words:
            raise ValueError(f"mask width {mask.shape[-1]} != the {self.mask_words} words of this memory's masks")
        return mask.reshape(-1, self.mask_words).to(self.device).contiguous()

    def _mask_index(self, mask_index, n_masks: int, Q: int) -> Optional[torch.Tensor]:
        """-> device int32 [Q] or ``None`` (one mask for all queries, or one per query)."""
        if mask_index is None:
            if n_masks not in (1, Q):
                raise ValueError(f"{n_masks} masks for {Q} queries need a mask_index")
            return None
        if isinstance(mask_index, torch.Tensor):
            if mask_index.dtype != torch.int32 or mask_index.dim() != 1:
                raise ValueError("a mask_index tensor must be int32 [Q]")
            idx = mask_index.to(self.device).contiguous()
        else:
            idx = torch.tensor([int(i) for i in mask_index], dtype=torch.int32).to(self.device)
        if idx.shape[0] != Q:
            raise ValueError(f"{idx.shape[0]} mask indices for {Q} queries")
        return idx

    def _one_mask(self, out) -> torch.Tensor:
        """The mask a builder writes: ``out`` (one mask, ``[W]`` or ``[1, W]``, on the device) or a new one."""
        if out is None:
            return self.new_mask()[0]
        if not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or out.numel() != self.mask_words or \
                out.device != self.device or not out.is_contiguous():
            raise ValueError(f"out must be one contiguous device int32 mask of {self.mask_words} words")
        return out

    def mask_of_rows(self, rows, out: Optional[torch.Tensor] = None, clear: bool = True) -> torch.Tensor:
        """-> the mask ``[W]`` of the live rows among ``rows``: a host sequence of row ids, or an int64 device tensor of
        any shape as a search returned it (it is NOT read on the host; the call is stream-ordered and capturable).  -1
        entries and ids of rows that are not live are skipped; duplicates are fine.  ``out``: the mask to write, default
        a new one; ``clear=False`` ORs the rows into what ``out`` holds."""
        if isinstance(rows, torch.Tensor):
            if rows.dtype != torch.int64:
                raise ValueError("row ids are int64")
            ids = rows.to(self.device).contiguous().view(-1)
        else:
            ids = torch.tensor([int(r) for r in rows], dtype=torch.int64).to(self.device)
        mask = self._one_mask(out)
        self.ctx.check(self.L.vm_mask_from_rows(self.handle, _ptr(ids), ids.numel(), 1, 0, 1 if clear else 0, _ptr(mask),
                                                _lib.current_stream_ptr()))
        _keep_alive(ids)
        return mask

    def mask_of_scope(self, scope, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> the mask ``[W]`` of the live rows of a tagged memory whose tag lies in ANY of the given inclusive ranges:
        one ``(lo, hi)``, a sequence of pairs, or an int64 ``[n, 2]`` tensor (``erase``'s selector).  Writes every word."""
        if not self.tagged:
            raise ValueError("mask_of_scope needs a tagged memory (EmbeddingMemory(..., tagged=True))")
        sc = self._scopes(scope)
        mask = self._one_mask(out)
        self.ctx.check(self.L.vm_mask_from_scopes(self.handle, _ptr(sc[0]), _ptr(sc[1]), sc.shape[1], _ptr(mask),
                                                  _lib.current_stream_ptr()))
        _keep_alive(sc)
        return mask

    def _live_rows(self) -> range:
        total = len(self)
        return range(total - self.capacity if self.ring and total > self.capacity else 0,
                     total if self.ring else min(total, self.capacity))

    def mask_where(self, fn) -> torch.Tensor:
        """-> the mask ``[W]`` of the live rows for which the host predicate ``fn(row, id, meta)`` holds (``id_of`` /
        ``meta_of`` of the row): a metadata filter.  Built on the host, one upload."""
        import numpy as np
        bits = np.zeros(self.mask_words * 32, dtype=np.uint8)
        for r in self._live_rows():
            if fn(r, self.id_of(r), self.meta_of(r)):
                bits[r % self.capacity] = 1
        words = np.packbits(bits, bitorder="little").view(np.uint32).view(np.int32)
        return torch.from_numpy(words.copy()).to(self.device)

    def rows_of_mask(self, mask: torch.Tensor) -> List[int]:
        """The live row ids one mask selects, ascending; decoded on the host (tests, debugging; synchronises)."""
        import numpy as np
        words = self._masks(mask)
        if words.shape[0] != 1:
            raise ValueError("rows_of_mask decodes one mask")
        bits = np.unpackbits(words[0].cpu().numpy().view(np.uint8), bitorder="little")
        return [r for r in self._live_rows() if bits[r % self.capacity]]

    def prepare_topk_masked(self, Q: int, k: int) -> MaskedTopkScratch:
        """Size the masked top-k workspace for (Q, k) now (before a graph capture: a capture must not allocate)."""
        return self._prepare_search(_MASKED, Q, k)

    def topk_masked(self, queries, k: int, mask, mask_index=None, min_score: Optional[float] = None,
                    score_mode: int = _lib.VM_SCORE_RAW, exact: bool = False,
                    scratch: Optional[MaskedTopkScratch] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (scores [Q,k] float64, rows [Q,k] int64): the k best rows among those a row mask selects, on any memory.
        ``mask``: int32 ``[W]`` (one mask for every query) or ``[n_masks, W]`` (``new_mask``, ``mask_of_rows``,
        ``mask_of_scope``, ``mask_where``, and ``& | ~`` of them); ``mask_index``: the mask each query uses (Q ints or a
        device int32 ``[Q]``), default mask 0 for all queries when there is one mask and mask q for query q when there are
        Q.  An index outside ``[0, n_masks)`` is the empty mask.

        The exhaustive row ranking of ``topk`` (score desc, row asc; score mapping and > min_score filter) over the
        selected live rows only; -1 / 0.0 padded.  Always the exhaustive answer: the fp32 fast path redoes the queries it
        cannot certify on the device, in the same call (csrc/topk_mask.hip).  ``exact=True`` scores every selected pair
        exactly (slow).  1 <= k <= 64.  The per-query flags of the last call (why a query was redone, vm_topk_flag) are in
        ``last_mask_flags``.  ``scratch``: as in ``topk`` - a ``MaskedTopkScratch`` the caller owns (a graph capture; a
        replay sees the mask as it is then), default this memory's own."""
        return self._search(_MASKED, queries, k, (mask, mask_index), min_score, score_mode, exact, scratch)

    # ---- row-id spans and recall links (include/vidmem.h vm_topk_cosine_span) ------------------------
    def prepare_topk_span(self, Q: int, k: int) -> SpanTopkScratch:
        """Size the span top-k workspace for (Q, k) now (before a graph capture: a capture must not allocate)."""
        return self._prepare_search(_SPAN, Q, k)

    @staticmethod
    def _open_spans(span):
        """``span`` as ``_scopes`` takes it: a tensor as it is (checked there), host pairs with ``None`` bounds opened."""
        if isinstance(span, torch.Tensor):
            return span
        def opened(p):
            if not hasattr(p, "__len__") or len(p) != 2:
                raise ValueError("a span is a pair (lo, hi)")
            return (INT64_MIN if p[0] is None else int(p[0]), INT64_MAX if p[1] is None else int(p[1]))
        pairs = list(span)
        if len(pairs) == 2 and not hasattr(pairs[0], "__len__"):
            return opened(pairs)
        return [opened(p) for p in pairs]

    def topk_span(self, queries, k: int, span, min_score: Optional[float] = None, score_mode: int = _lib.VM_SCORE_RAW,
                  exact: bool = False, scratch: Optional[SpanTopkScratch] = None, stride: Tuple[int, int] = (1, 0)
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (scores [Q,k] float64, rows [Q,k] int64): the k best rows among those whose ROW ID lies in the query's span,
        on any memory.  Row ids are append order, so a span is a stretch of time: "the past before this frame".
        ``span``: one inclusive ``(lo, hi)`` for all queries, a sequence of Q pairs, or a device int64 ``[Q, 2]`` tensor
        (not read on the host; a captured call sees it rewritten in place).  ``None`` as a bound means open.  The ids
        are this memory's own (before ``stride``); ids that name no live row are ignored, ``lo > hi`` is the empty span.

        The exhaustive row ranking of ``topk`` (score desc, row asc; score mapping and > min_score filter) over the rows
        in the span only; -1 / 0.0 padded.  Always the exhaustive answer: the fp32 fast path redoes the queries it cannot
        certify on the device, in the same call (csrc/topk_span.hip).  ``exact=True`` scores every in-span pair exactly
        (slow).  1 <= k <= 64.  ``stride``: ``(row_stride, row_offset)`` of the returned ids, as in ``topk``.  The
        per-query flags of the last call are in ``last_span_flags``.  ``scratch``: as in ``topk`` - a ``SpanTopkScratch``
        the caller owns (a graph capture), default this memory's own.  A span speaks about row ids: after an erase it is
        stale exactly as a mask is."""
        return self._search(_SPAN, queries, k, self._open_spans(span), min_score, score_mode, exact, scratch, stride)

    def recall_links(self, first_row: Optional[int] = None, n_rows: Optional[int] = None, k: int = 10, min_gap: int = 1,
                     max_back: Optional[int] = None, exclude_group: bool = False, min_score: Optional[float] = None,
                     score_mode: int = _lib.VM_SCORE_RAW, block: int = 256, exact: bool = False
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (scores [n_rows,k] float64, rows [n_rows,k] int64): for each stored row, its k best matches in ITS OWN PAST.
        Query i is the stored row ``r = first_row + i`` (default: every live row) and its span is
        ``[r - max_back, r - min_gap]``, open below when ``max_back`` is ``None``; ``min_gap >= 1`` keeps the row itself
        and its nearest temporal neighbours out.  ``exclude_group=True`` (grouped memories only): the span also ends no
        later than the row before the first row of r's own group, so a row never links into its own chunk or event.
        Rows with an empty past come back all-padded (-1 / 0.0).

        Everything is built on the device and searched with ``topk_span``, in pages of ``block`` consecutive rows: a
        page's spans end below its last row, so the tiles behind it are skipped for free and a whole-memory pass scores
        about half the pairs.  One page needs ``4 x block x capacity`` bytes of workspace plus the fixed part.  Reads the
        host row count: after captured appends call ``sync()`` first."""
        k, min_gap, block = int(k), int(min_gap), int(block)
        if min_gap < 1:
            raise ValueError(f"recall_links needs min_gap >= 1 (a row always matches itself), got {min_gap}")
        if max_back is not None and int(max_back) < 0:
            raise ValueError(f"max_back must be >= 0 or None, got {max_back}")
        if block < 1:
            raise ValueError(f"block must be >= 1, got {block}")
        if not 1 <= k <= 64:
            raise ValueError(f"span top-k supports 1 <= k <= 64, got {k}")
        if exclude_group and not self.grouped:
            raise ValueError("exclude_group=True needs a grouped memory (EmbeddingMemory(..., grouped=True))")
        total, n = len(self), self.searchable
        base = total - n
        first = base if first_row is None else int(first_row)
        count = total - first if n_rows is None else int(n_rows)
        if first < base or count < 0 or first + count > total:
            raise ValueError(f"rows {first} .. {first + count - 1} are not all live ({base} .. {total - 1} are)")
        scores = torch.zeros((count, k), dtype=torch.float64, device=self.device)
        rows = torch.full((count, k), -1, dtype=torch.int64, device=self.device)
        if count == 0:
            return scores, rows
        table = self.rows_tensor()
        if exclude_group:      # ordinals rise by 0 or 1 from each row to the next: a group's first row by bisection
            col = _tensor_from_ptr(self.L.vm_memory_group_ordinals(self.handle), (n,), torch.int64, self.device)
            ords = self._in_row_order(col).contiguous()
        for b0 in range(0, count, block):
            r = torch.arange(first + b0, first + min(b0 + block, count), dtype=torch.int64, device=self.device)
            hi = r - min_gap
            lo = torch.full_like(r, INT64_MIN) if max_back is None else r - int(max_back)
            if exclude_group:
                group_first = base + torch.searchsorted(ords, ords[r - base])
                hi = torch.minimum(hi, group_first - 1)
            s, got = self.topk_span(table[self._slots_of(r)], k, torch.stack([lo, hi], dim=1), min_score=min_score,
                                    score_mode=score_mode, exact=exact)
            scores[b0:b0 + r.numel()] = s
            rows[b0:b0 + r.numel()] = got
        return scores, rows

    # ---- mixed-query search (include/vidmem.h vm_topk_cosine_mix) -----------------------------------
    def prepare_topk_mix(self, C: int, J: int, k: int) -> MixTopkScratch:
        """Size the mixed top-k workspace for ``C`` mixed queries of ``J`` terms and ``k`` hits each now (before a graph
        capture: a capture must not allocate).  The workspace does not depend on ``J``: a query's terms always fill
        one 16-column tile."""
        if not 1 <= int(J) <= 16:
            raise ValueError(f"mixed top-k supports 1 <= J <= 16 terms, got {J}")
        return self._prepare_search(_MIX, C, k)

    def _mix_terms(self, terms) -> torch.Tensor:
        """-> contiguous device ``[C, J, D]`` in the memory's dtype from ``[C, J, D]`` or ``[J, D]`` (one query)."""
        if not isinstance(terms, torch.Tensor):
            terms = torch.tensor(terms, dtype=torch.float32)
        if terms.dim() == 2:
            terms = terms.unsqueeze(0)
        if terms.dim() != 3 or terms.shape[-1] != self.dim:
            raise ValueError(f"terms must be [C, J, {self.dim}] or [J, {self.dim}], got {tuple(terms.shape)}")
        if terms.shape[0] < 1:
            raise ValueError("no mixed query")
        if not 1 <= terms.shape[1] <= 16:
            raise ValueError(f"mixed top-k supports 1 <= J <= 16 terms, got {terms.shape[1]}")
        return terms.to(device=self.device, dtype=self.dtype).contiguous()

    def _mix_weights(self, weights, Cn: int, J: int) -> torch.Tensor:
        """-> contiguous device float64 ``[C, J]`` from a tensor, a nested list, or one list of J shared by all C."""
        w = weights if isinstance(weights, torch.Tensor) else torch.tensor(weights, dtype=torch.float64)
        if w.dim() == 1:
            w = w.unsqueeze(0).expand(Cn, -1)
        if tuple(w.shape) != (Cn, J):
            raise ValueError(f"weights must be [{Cn}, {J}] or one list of {J}, got {tuple(w.shape)}")
        return w.to(device=self.device, dtype=torch.float64).contiguous()

    def topk_mix(self, terms, weights, k: int, mask=None, mask_index=None, min_score: Optional[float] = None,
                 exact: bool = False, scratch: Optional[MixTopkScratch] = None, stride: Tuple[int, int] = (1, 0)
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (scores [C,k] float64, rows [C,k] int64): the k best rows by a WEIGHTED SUM OF COSINES, on any memory.
        ``terms``: ``[C, J, D]`` (or ``[J, D]`` for one query), J <= 16 vectors per mixed query; ``weights``: a float64
        tensor ``[C, J]``, a nested list, or one list of J shared by all C - positive, negative or zero.  The score of
        row r is ``W = sum_j w_j * cos(term_j, r)``: the reference's fp64 cosines, summed left to right from 0.0 with one
        rounding per product and per addition, so ``J = 1, w = 1`` is ``topk`` bit for bit and zero-weight terms change
        nothing.  ``mask`` / ``mask_index``: as in ``topk_masked`` with one mask per mixed query, default every live
        row; an exclusion is ``~mask_of_rows(rows_already_shown)``.

        Ranked by (W desc, row id asc), the optional strict ``W > min_score`` filter on the raw sum (there is no score
        mapping: W is not confined to [-1, 1]), -1 / 0.0 padded; ``stride``: the ``(row_stride, row_offset)`` of the
        returned ids.  Always the exhaustive answer: the fp32 fast path redoes the queries it cannot certify on the
        device, in the same call (csrc/topk_mix.hip).  ``exact=True`` scores every selected pair exactly (slow).  The
        per-query flags of the last fast call are in ``last_mix_flags``.  ``scratch``: as in ``topk`` - a
        ``MixTopkScratch`` the caller owns (a graph capture: pass ``terms``, ``weights`` and ``mask`` as device tensors
        of their final dtype and rewrite them in place between replays), default this memory's own."""
        def operands(_):
            q = self._mix_terms(terms)
            Cn, J = int(q.shape[0]), int(q.shape[1])
            w = self._mix_weights(weights, Cn, J)
            return Cn, (_ptr(q), _ptr(w), Cn, J, int(k)), (q, w)
        return self._scored(_MIX, k, operands, mask, mask_index, min_score, exact, scratch, stride)

    # ---- any/all search: the max or min of weighted cosines (include/vidmem.h vm_topk_cosine_fold) ----
    def prepare_topk_fold(self, C: int, J: int, k: int) -> FoldTopkScratch:
        """Size the any/all top-k workspace for ``C`` fold queries of ``J`` terms and ``k`` hits each now (before a graph
        capture: a capture must not allocate).  The workspace does not depend on ``J``: a query's terms always fill
        one 16-column tile."""
        if not 1 <= int(J) <= 16:
            raise ValueError(f"any/all top-k supports 1 <= J <= 16 terms, got {J}")
        return self._prepare_search(_FOLD, C, k)

    def topk_fold(self, terms, k: int, op: str = "max", weights=None, mask=None, mask_index=None,
                  min_score: Optional[float] = None, exact: bool = False, scratch: Optional[FoldTopkScratch] = None,
                  stride: Tuple[int, int] = (1, 0)) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """-> (scores [C,k] float64, rows [C,k] int64, terms_idx [C,k] int32): the k best rows by the MAXIMUM
        (``op="max"``, any / OR) or the MINIMUM (``op="min"``, all / AND) of the weighted cosines over a query's terms,
        on any memory.  ``terms``: ``[C, J, D]`` (or ``[J, D]`` for one query), J <= 16; ``weights``: as in ``topk_mix``,
        ``None`` = all 1.0.  The score of row r is ``F = max_j / min_j (w_j * cos(term_j, r))`` over the reference's fp64
        cosines, one rounding per product, a strict compare taken j = 0 .. J-1: the first term wins a tie, and
        ``terms_idx`` names it (which frame linked, which question matched; -1 where the row is -1).  ``J = 1, w = 1`` is
        ``topk`` bit for bit; a permutation of the terms changes only ``terms_idx`` (and the sign of a score that is a
        zero: products that tie as +0.0 and -0.0 give F the sign of the first); a repeated term changes nothing.  A
        ZERO WEIGHT IS NOT NEUTRAL, unlike in ``topk_mix``: its product +-0.0 takes part in the max / min.

        Ranked by (F DESCENDING, row id ascending) for both ops - ``"min"`` returns the rows whose worst term is best -,
        the optional strict ``F > min_score`` filter on the raw value, -1 / 0.0 padded; ``mask`` / ``mask_index``,
        ``stride``, ``exact`` and ``scratch`` (a ``FoldTopkScratch``) as in ``topk_mix``.  Always the exhaustive answer:
        the fp32 fast path redoes the queries it cannot certify on the device, in the same call (csrc/topk_mix.hip); the
        per-query flags of the last fast call are in ``last_fold_flags``."""
        if op not in ("max", "min"):
            raise ValueError(f"op must be 'max' or 'min', got {op!r}")
        def operands(_):
            q = self._mix_terms(terms)
            Cn, J = int(q.shape[0]), int(q.shape[1])
            w = self._mix_weights([1.0] * J if weights is None else weights, Cn, J)
            return Cn, (_ptr(q), _ptr(w), Cn, J, int(k), _lib.VM_FOLD_MAX if op == "max" else _lib.VM_FOLD_MIN), (q, w)
        return self._scored(_FOLD, k, operands, mask, mask_index, min_score, exact, scratch, stride)

    def topk_any(self, terms, k: int, **kw) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``topk_fold(terms, k, op="max", ...)``: the rows that resemble ANY term."""
        return self.topk_fold(terms, k, op="max", **kw)

    def topk_all(self, terms, k: int, **kw) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``topk_fold(terms, k, op="min", ...)``: the rows that resemble ALL terms (ranked by their worst one)."""
        return self.topk_fold(terms, k, op="min", **kw)

    # ---- biased search: cosine plus a per-row prior (include/vidmem.h vm_topk_cosine_biased) --------
    @property
    def bias_stride(self) -> int:
        """S: the fp32 entries of one bias column of this memory (``vm_memory_bias_stride``: the capacity rounded up to
        64 rows, = 32 x ``mask_words``)."""
        return self.mask_words * 32

    def new_bias(self, n: int = 1) -> torch.Tensor:
        """-> device float32 zeros ``[n, S]``: ``n`` bias columns.  The entry of row id ``r`` is entry ``r % capacity``;
        entries of slots without a live row are ignored by every consumer, so a column may be filled by any torch
        expression.  A column speaks about ROW IDS: after an erase or a ring overwrite it is stale exactly as a mask
        is."""
        return torch.zeros((int(n), self.bias_stride), dtype=torch.float32, device=self.device)

    def _biases(self, bias) -> torch.Tensor:
        """-> contiguous device float32 ``[n_bias, S]`` from one column ``[S]`` or several ``[n_bias, S]``: a device
        tensor of that form is passed through untouched, anything else is refused before the library is called."""
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32:
            raise ValueError("a bias is a float32 tensor (EmbeddingMemory.new_bias)")
        if bias.dim() not in (1, 2) or bias.shape[0] == 0:
            raise ValueError(f"a bias is [S] or [n_bias, S] with n_bias >= 1, got {tuple(bias.shape)}")
        if bias.shape[-1] != self.bias_stride:
            raise ValueError(f"bias width {bias.shape[-1]} != the {self.bias_stride} entries of this memory's columns")
        if bias.device != self.device:
            raise ValueError(f"the bias is on {bias.device}, the memory on {self.device}")
        return bias.reshape(-1, self.bias_stride).contiguous()

    def _bias_index(self, bias_index, n_bias: int, Q: int) -> Optional[torch.Tensor]:
        """-> device int32 [Q] or ``None`` (one column for all queries, or one per query)."""
        if bias_index is None:
            if n_bias not in (1, Q):
                raise ValueError(f"{n_bias} bias columns for {Q} queries need a bias_index")
            return None
        if isinstance(bias_index, torch.Tensor):
            if bias_index.dtype != torch.int32 or bias_index.dim() != 1:
                raise ValueError("a bias_index tensor must be int32 [Q]")
            idx = bias_index.to(self.device).contiguous()
        else:
            idx = torch.tensor([int(i) for i in bias_index], dtype=torch.int32).to(self.device)
        if idx.shape[0] != Q:
            raise ValueError(f"{idx.shape[0]} bias indices for {Q} queries")
        return idx

    def _bias_weight(self, weight, Q: int) -> Optional[torch.Tensor]:
        """-> device float64 [Q] or ``None`` (1.0 for every query) from a tensor, one number or Q numbers."""
        if weight is None:
            return None
        if isinstance(weight, torch.Tensor):
            if weight.dtype != torch.float64 or weight.dim() != 1:
                raise ValueError("a weight tensor must be float64 [Q]")
            w = weight.to(self.device).contiguous()
        else:
            vals = [float(weight)] * Q if not hasattr(weight, "__len__") else [float(x) for x in weight]
            w = torch.tensor(vals, dtype=torch.float64).to(self.device)
        if w.shape[0] != Q:
            raise ValueError(f"{w.shape[0]} weights for {Q} queries")
        return w

    def _one_bias(self, out) -> torch.Tensor:
        """The column a builder writes: ``out`` (one column, ``[S]`` or ``[1, S]``, on the device) or a new one."""
        if out is None:
            return self.new_bias()[0]
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.numel() != self.bias_stride or \
                out.device != self.device or not out.is_contiguous():
            raise ValueError(f"out must be one contiguous device float32 column of {self.bias_stride} entries")
        return out

    def bias_of_rows(self, rows, values, out: Optional[torch.Tensor] = None, clear: bool = True) -> torch.Tensor:
        """-> the column ``[S]`` that holds ``values[i]`` for every live row ``rows[i]``: a prior from the hits of another
        search or of another retrieval leg.  ``rows``: a host sequence of row ids, or an int64 device tensor of any shape
        as a search returned it (NOT read on the host; stream-ordered and capturable); ``values``: as many float32
        values (a device tensor, a host sequence, or one number for all).  -1 entries and ids of rows that are not live
        are skipped; of duplicates that carry different values one stays.  ``out``: the column to write, default a new
        one; ``clear=False`` leaves the other entries of ``out`` as they are."""
        if isinstance(rows, torch.Tensor):
            if rows.dtype != torch.int64:
                raise ValueError("row ids are int64")
            ids = rows.to(self.device).contiguous().view(-1)
        else:
            ids = torch.tensor([int(r) for r in rows], dtype=torch.int64).to(self.device)
        if isinstance(values, torch.Tensor):
            if values.dtype != torch.float32:
                raise ValueError("bias values are float32")
            vals = values.to(self.device).contiguous().view(-1)
        elif hasattr(values, "__len__"):
            vals = torch.tensor([float(v) for v in values], dtype=torch.float32).to(self.device)
        else:
            vals = torch.full((ids.numel(),), float(values), dtype=torch.float32, device=self.device)
        if vals.numel() != ids.numel():
            raise ValueError(f"{vals.numel()} values for {ids.numel()} rows")
        col = self._one_bias(out)
        self.ctx.check(self.L.vm_bias_from_rows(self.handle, _ptr(ids), _ptr(vals), ids.numel(), 1, 0, 1 if clear else 0,
                                                _ptr(col), _lib.current_stream_ptr()))
        _keep_alive(ids, vals)
        return col

    def bias_of_age(self, now_ms: int, per_ms: float, fill: float = 0.0, out: Optional[torch.Tensor] = None
                    ) -> torch.Tensor:
        """-> the column ``[S]`` of linear recency on a tagged memory: a live row tagged with ``ms`` milliseconds gets
        ``float32(per_ms * (ms - now_ms))`` - with ``per_ms = 1e-6`` a frame loses 0.06 of score per minute of age -,
        untagged rows and slots without a live row get ``fill``.  Writes every entry; any other shape of decay is a
        torch expression over the result."""
        if not self.tagged:
            raise ValueError("bias_of_age needs a tagged memory (EmbeddingMemory(..., tagged=True))")
        col = self._one_bias(out)
        self.ctx.check(self.L.vm_bias_from_tags(self.handle, int(now_ms), float(per_ms), float(fill), _ptr(col),
                                                _lib.current_stream_ptr()))
        return col

    def prepare_topk_biased(self, Q: int, k: int) -> BiasTopkScratch:
        """Size the biased top-k workspace for (Q, k) now (before a graph capture: a capture must not allocate)."""
        return self._prepare_search(_BIASED, Q, k)

    def topk_biased(self, queries, k: int, bias, weight=None, bias_index=None, mask=None, mask_index=None,
                    min_score: Optional[float] = None, exact: bool = False, scratch: Optional[BiasTopkScratch] = None,
                    stride: Tuple[int, int] = (1, 0)) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (scores [Q,k] float64, rows [Q,k] int64): the k best rows by COSINE PLUS A PER-ROW PRIOR, on any memory.
        ``bias``: float32 ``[S]`` (one column for every query) or ``[n_bias, S]`` (``new_bias``, ``bias_of_rows``,
        ``bias_of_age``, or any torch expression); ``bias_index``: the column each query uses (Q ints or a device int32
        ``[Q]``), default column 0 for all queries when there is one and column q for query q when there are Q; an index
        outside ``[0, n_bias)`` is the zero column.  ``weight``: beta per query - one number, Q numbers or a device
        float64 ``[Q]`` -, default 1.0.  The score of row r is ``S = cos(q, r) + beta * bias[r % capacity]``: the
        reference's fp64 cosine, the bias widened exactly, one rounding for the product and one for the sum, so
        ``beta = 0`` or a column of zeros is ``topk`` (with a mask: ``topk_masked``) bit for bit.  ``mask`` /
        ``mask_index``: as in ``topk_masked``, default every live row.

        Ranked by (S desc, row id asc), the optional strict ``S > min_score`` filter on the raw sum (there is no score
        mapping: S is not confined to [-1, 1]), -1 / 0.0 padded; ``stride``: the ``(row_stride, row_offset)`` of the
        returned ids.  Always the exhaustive answer: the fp32 fast path redoes the queries it cannot certify on the
        device, in the same call (csrc/topk_bias.hip).  ``exact=True`` scores every selected pair exactly (slow).  The
        per-query flags of the last fast call are in ``last_bias_flags``.  ``scratch``: as in ``topk`` - a
        ``BiasTopkScratch`` the caller owns (a graph capture: pass ``queries``, ``bias``, ``weight``, ``bias_index`` and
        ``mask`` as device tensors of their final dtype and rewrite them in place between replays), default this
        memory's own."""
        def operands(cols):
            q = self._as_rows(queries)
            Q = int(q.shape[0])
            if Q < 1:
                raise ValueError("no query")
            bidx = self._bias_index(bias_index, cols.shape[0], Q)
            w = self._bias_weight(weight, Q)
            return Q, (_ptr(q), Q, int(k), _ptr(cols), cols.shape[0], _ptr(bidx), _ptr(w)), (q, cols, bidx, w)
        return self._scored(_BIASED, k, operands, mask, mask_index, min_score, exact, scratch, stride,
                            first=lambda: self._biases(bias))

    # ---- diverse search (include/vidmem.h vm_topk_cosine_diverse) ------------------------------------
    @staticmethod
    def _diverse_pool(k, pool) -> Tuple[int, int]:
        """-> (k, pool) of a diverse call, the default pool ``min(64, max(k, 4 k))`` filled in; refused when they are not
        ``1 <= k <= pool <= 64``."""
        k = int(k)
        pool = min(64, max(k, 4 * k)) if pool is None else int(pool)
        if not 1 <= k <= 64:
            raise ValueError(f"diverse top-k supports 1 <= k <= 64, got {k}")
        if pool > 64:
            raise ValueError(f"diverse top-k supports pool <= 64, got {pool}")
        if k > pool:
            raise ValueError(f"diverse top-k needs k <= pool, got k={k}, pool={pool}")
        return k, pool

    def prepare_topk_diverse(self, Q: int, k: int, pool: Optional[int] = None) -> DiverseTopkScratch:
        """Size the diverse top-k workspace for ``Q`` queries, ``k`` picks and a pool of ``pool`` rows each now (before a
        graph capture: a capture must not allocate).  The workspace depends on ``Q`` and ``pool`` only."""
        k, pool = self._diverse_pool(k, pool)
        return self._prepare_search(_DIVERSE, Q, pool)

    def _diverse_lam(self, lam, Q: int) -> torch.Tensor:
        """-> contiguous device float64 ``[Q]``.  A device float64 tensor passes through unread (a captured call sees it
        rewritten in place); a float or Q floats are checked to lie in [0, 1] here."""
        if isinstance(lam, torch.Tensor) and lam.is_cuda:
            if lam.dtype != torch.float64 or tuple(lam.shape) != (Q,):
                raise ValueError(f"a device lam must be float64 [{Q}], got {lam.dtype} {tuple(lam.shape)}")
            return lam.to(self.device).contiguous()
        vals = lam.tolist() if isinstance(lam, torch.Tensor) else lam
        vals = [float(v) for v in vals] if hasattr(vals, "__len__") else [float(vals)] * Q
        if len(vals) != Q:
            raise ValueError(f"{len(vals)} values of lam for {Q} queries")
        for v in vals:
            if not 0.0 <= v <= 1.0:     # NaN included
                raise ValueError(f"lam must lie in [0, 1], got {v}")
        return torch.tensor(vals, dtype=torch.float64).to(self.device)

    def topk_diverse(self, queries, k: int, pool: Optional[int] = None, lam=0.5, mask=None, mask_index=None,
                     min_score: Optional[float] = None, exact: bool = False,
                     scratch: Optional[DiverseTopkScratch] = None, stride: Tuple[int, int] = (1, 0)
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (scores [Q,k] float64, rows [Q,k] int64): k DIVERSE hits per query by maximal marginal relevance, on any
        memory.  The pool is the query's ``pool`` best rows (``topk``'s ranking over the rows ``mask`` selects, strict
        ``> min_score`` on the raw cosine; default ``pool = min(64, max(k, 4 k))``).  The first pick is the best row; each
        later pick is the unpicked pool row with the largest ``lam * e - (1 - lam) * max sim(row, picked)``, ``e`` its
        cosine with the query and ``sim`` the reference cosine between two STORED rows, every operation rounded once in
        fp64, ties to the smaller row id (include/vidmem.h).  ``lam = 1`` is ``topk`` / ``topk_masked`` bit for bit,
        ``lam = 0`` cares for spread alone after the first pick.  Rows come in PICK order with their relevance ``e`` as
        score, -1 / 0.0 padded; the value each was picked at is in ``last_diverse_mmr``.

        ``lam``: a float, Q floats, or a device float64 ``[Q]`` tensor, which is passed through unread.  A host value
        outside [0, 1], ``k > pool`` or ``pool > 64`` raises ``ValueError`` before the library is called.  ``mask`` /
        ``mask_index``: as in ``topk_masked``, default every live row.  ``stride``: the ``(row_stride, row_offset)`` of the
        returned ids.  The pool is always the exhaustive answer (its fast path redoes what it cannot certify on the
        device; ``last_diverse_flags``, ``diverse_uncertified_count``); ``exact=True`` scores every selected pair exactly
        (slow).  ``scratch``: as in ``topk`` - a ``DiverseTopkScratch`` the caller owns (a graph capture: pass
        ``queries``, ``lam`` and ``mask`` as device tensors of their final dtype and rewrite them in place between
        replays), default this memory's own."""
        k, pool = self._diverse_pool(k, pool)

        def operands(_):
            q = self._as_rows(queries)
            Q = int(q.shape[0])
            lm = self._diverse_lam(lam, Q)
            return Q, (_ptr(q), Q, k, pool, _ptr(lm)), (q, lm)
        scores, rows = self._scored(_DIVERSE, k, operands, mask, mask_index, min_score, exact, scratch, stride,
                                    sized_by=pool)
        self._last_diverse_shape = (scores.shape[0], k)
        return scores, rows

    @property
    def last_diverse_mmr(self) -> Optional[torch.Tensor]:
        """float64 ``[Q, k]``: the value ``lam * e - (1 - lam) * red`` at which each row of the last ``topk_diverse``
        call was picked, 0.0 padded (a view of the scratch that call used; ``None`` before the first call)."""
        s = self._last.get(DiverseTopkScratch)
        if s is None:
            return None
        Q, k = self._last_diverse_shape
        return s.mmr[:Q * k].view(Q, k)

    # ---- clip search (include/vidmem.h vm_topk_cosine_clip) -----------------------------------------
    def prepare_topk_clip(self, C: int, L: int, k: int) -> "ClipScratch":
        """Size this memory's own clip-search buffers for ``C`` clips of ``L`` frames and ``k`` hits each now (before a
        graph capture: a capture must not allocate)."""
        self._counter(ClipScratch)
        return self._resolve(ClipScratch, None, int(C), int(L), int(k))

    def _clip_args(self, clips, k, min_sep, scope, max_gap_ms, min_score, score_mode):
        if not isinstance(clips, torch.Tensor):
            clips = torch.tensor(clips, dtype=torch.float32)
        if clips.dim() == 2:
            clips = clips.unsqueeze(0)
        if clips.dim() != 3 or clips.shape[-1] != self.dim:
            raise ValueError(f"clips must be [C, L, {self.dim}] or [L, {self.dim}], got {tuple(clips.shape)}")
        Cn, L = int(clips.shape[0]), int(clips.shape[1])
        if Cn < 1:
            raise ValueError("no clip")
        if not 1 <= L <= 16:
            raise ValueError(f"clip search supports 1 <= L <= 16 frames, got {L}")
        if not 1 <= int(k) <= 64:
            raise ValueError(f"clip search supports 1 <= k <= 64, got {k}")
        sep = L if min_sep is None else int(min_sep)
        if not 1 <= sep <= 32:
            raise ValueError(f"clip search supports 1 <= min_sep <= 32, got {sep}")
        if score_mode not in (_lib.VM_SCORE_RAW, _lib.VM_SCORE_UNIT_INTERVAL):
            raise ValueError("score_mode must be VM_SCORE_RAW or VM_SCORE_UNIT_INTERVAL")
        if (scope is not None or (max_gap_ms is not None and int(max_gap_ms) >= 0)) and not self.tagged:
            raise ValueError("scope and max_gap_ms need a tagged memory (EmbeddingMemory(..., tagged=True))")
        if min_score is not None and math.isnan(float(min_score)):
            raise ValueError("min_score is NaN")
        q = clips.to(device=self.device, dtype=self.dtype).contiguous()
        sc = self._scopes(scope, Cn) if scope is not None else None
        gap = -1 if max_gap_ms is None else int(max_gap_ms)
        return q, Cn, L, sep, sc, gap

    def enqueue_topk_clip(self, clips, k: int, min_sep: Optional[int] = None, scope=None,
                          max_gap_ms: Optional[int] = None, min_score: Optional[float] = None,
                          score_mode: int = _lib.VM_SCORE_RAW, scratch: Optional["ClipScratch"] = None,
                          exact: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """The capturable clip search -> ``(scores [C,k] float64, rows [C,k] int64)``: views of the buffers of
        ``scratch`` (default: this memory's own, ``prepare_topk_clip``), valid until the next clip call on it.  Arguments
        as in ``topk_clip``.  Enqueues ``vm_topk_cosine_clip`` on the current stream: nothing is read on the host.
        Inside a graph capture pass ``clips`` as a device tensor of the memory's dtype and ``scope`` as an int64
        ``[C, 2]`` device tensor (both rewritten in place between replays) and a ``scratch`` the session owns, or call
        ``prepare_topk_clip`` first."""
        q, Cn, L, sep, sc, gap = self._clip_args(clips, k, min_sep, scope, max_gap_ms, min_score, score_mode)
        k = int(k)
        scratch = self._resolve(ClipScratch, scratch, Cn, L, k)
        scores = scratch.scores[:Cn * k].view(Cn, k)
        rows = scratch.rows[:Cn * k].view(Cn, k)
        lo, hi = (sc[0], sc[1]) if sc is not None else (None, None)
        head = (self.handle, _ptr(q), Cn, L, k, sep, gap, _ptr(lo), _ptr(hi), *_min_score_args(min_score),
                int(score_mode), _ptr(scores), _ptr(rows))
        tail = (_ptr(scratch.ws), scratch.ws.numel(), _lib.current_stream_ptr())
        if exact:
            self.ctx.check(self.L.vm_topk_cosine_clip_exact(*head, *tail))
        else:
            self.ctx.check(self.L.vm_topk_cosine_clip(*head, _ptr(self._counter(ClipScratch)), _ptr(scratch.flags),
                                                      *tail))
        _keep_alive(q, sc)
        self._last[ClipScratch] = scratch
        return scores, rows

    def topk_clip(self, clips, k: int, min_sep: Optional[int] = None, scope=None, max_gap_ms: Optional[int] = None,
                  min_score: Optional[float] = None, score_mode: int = _lib.VM_SCORE_RAW, exact: bool = False
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (scores [C,k] float64, rows [C,k] int64): where each clip - a SEQUENCE of L <= 16 frames, ``clips``
        ``[C,L,D]`` or ``[L,D]`` - occurs in the memory.  ``rows`` are START row ids: window r is the rows r .. r+L-1 and
        scores the mean of the L aligned reference cosines (frame i against row r+i; the fp64 values bit for bit).

        A window must lie within the live rows and, on a tagged memory, within one video (no change of source inside;
        ``max_gap_ms``: no clock step backwards or above it either); with ``scope`` (one ``(lo, hi)`` or C pairs, as
        in ``topk_scoped``) every one of its rows must be in scope.  The k answers are PEAKS: windows that rank before
        every other such window closer than ``min_sep`` rows (default: L, non-overlapping windows; 1 = every window), in
        (score desc, start asc) - local-maximum suppression, so k answers are k moments, not k shifts of one.  Score
        mapping and strict ``> min_score`` filter as in ``topk``; -1 / 0.0 padded.  Always the exhaustive answer: the
        fp32 fast path redoes the clips it cannot certify on the device, in the same call (csrc/topk_clip.hip).
        ``exact=True`` scores every window exactly (slow).  The per-clip flags of the last call are in
        ``last_clip_flags``."""
        scores, rows = self.enqueue_topk_clip(clips, k, min_sep=min_sep, scope=scope, max_gap_ms=max_gap_ms,
                                              min_score=min_score, score_mode=score_mode, exact=exact)
        return scores.clone(), rows.clone()

    # ---- sequence search (include/vidmem.h vm_topk_cosine_seq) --------------------------------------
    def prepare_topk_seq(self, C: int, J: int, k: int) -> "SeqScratch":
        """Size this memory's own sequence-search buffers for ``C`` sequences of ``J`` steps and ``k`` hits each now
        (before a graph capture: a capture must not allocate)."""
        self._counter(SeqScratch)
        return self._resolve(SeqScratch, None, int(C), int(J), int(k))

    def _seq_args(self, steps, k, max_step, min_sep, mask, mask_index, max_gap_ms, min_score, score_mode):
        if not isinstance(steps, torch.Tensor):
            steps = torch.tensor(steps, dtype=torch.float32)
        if steps.dim() == 2:
            steps = steps.unsqueeze(0)
        if steps.dim() != 3 or steps.shape[-1] != self.dim:
            raise ValueError(f"steps must be [C, J, {self.dim}] or [J, {self.dim}], got {tuple(steps.shape)}")
        Cn, J = int(steps.shape[0]), int(steps.shape[1])
        if Cn < 1:
            raise ValueError("no sequence")
        if not 1 <= J <= 16:
            raise ValueError(f"sequence search supports 1 <= J <= 16 steps, got {J}")
        if not 1 <= int(k) <= 64:
            raise ValueError(f"sequence search supports 1 <= k <= 64, got {k}")
        G = int(max_step)
        if not 1 <= G <= 16:
            raise ValueError(f"sequence search supports 1 <= max_step <= 16, got {G}")
        sep = min(32, (J - 1) * G + 1) if min_sep is None else int(min_sep)
        if not 1 <= sep <= 32:
            raise ValueError(f"sequence search supports 1 <= min_sep <= 32, got {sep}")
        if score_mode not in (_lib.VM_SCORE_RAW, _lib.VM_SCORE_UNIT_INTERVAL):
            raise ValueError("score_mode must be VM_SCORE_RAW or VM_SCORE_UNIT_INTERVAL")
        if max_gap_ms is not None and int(max_gap_ms) >= 0 and not self.tagged:
            raise ValueError("max_gap_ms needs a tagged memory (EmbeddingMemory(..., tagged=True))")
        if min_score is not None and math.isnan(float(min_score)):
            raise ValueError("min_score is NaN")
        masks = self._masks(mask) if mask is not None else None
        if masks is None and mask_index is not None:
            raise ValueError("a mask_index needs a mask")
        idx = self._mask_index(mask_index, masks.shape[0], Cn) if masks is not None else None
        q = steps.to(device=self.device, dtype=self.dtype).contiguous()
        gap = -1 if max_gap_ms is None else int(max_gap_ms)
        return q, Cn, J, G, sep, masks, idx, gap

    def enqueue_topk_seq(self, steps, k: int, max_step: int = 4, min_sep: Optional[int] = None, mask=None,
                         mask_index=None, max_gap_ms: Optional[int] = None, min_score: Optional[float] = None,
                         score_mode: int = _lib.VM_SCORE_RAW, scratch: Optional["SeqScratch"] = None,
                         exact: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """The capturable sequence search -> ``(scores [C,k] float64, rows [C,k] int64, step_rows [C,k,J] int64,
        step_scores [C,k,J] float64)``: views of the buffers of ``scratch`` (default: this memory's own,
        ``prepare_topk_seq``), valid until the next sequence call on it.  Arguments as in ``topk_seq``.  Enqueues
        ``vm_topk_cosine_seq`` on the current stream: nothing is read on the host.  Inside a graph capture pass ``steps``
        as a device tensor of the memory's dtype and ``mask`` / ``mask_index`` as device tensors (all rewritten in place
        between replays) and a ``scratch`` the session owns, or call ``prepare_topk_seq`` first."""
        q, Cn, J, G, sep, masks, idx, gap = self._seq_args(steps, k, max_step, min_sep, mask, mask_index, max_gap_ms,
                                                           min_score, score_mode)
        k = int(k)
        scratch = self._resolve(SeqScratch, scratch, Cn, J, k)
        scores = scratch.scores[:Cn * k].view(Cn, k)
        rows = scratch.rows[:Cn * k].view(Cn, k)
        step_rows = scratch.step_rows[:Cn * k * J].view(Cn, k, J)
        step_scores = scratch.step_scores[:Cn * k * J].view(Cn, k, J)
        head = (self.handle, _ptr(q), Cn, J, k, G, sep, gap, _ptr(masks), 0 if masks is None else masks.shape[0],
                _ptr(idx), *_min_score_args(min_score), int(score_mode), _ptr(scores), _ptr(rows), _ptr(step_rows),
                _ptr(step_scores))
        tail = (_ptr(scratch.ws), scratch.ws.numel(), _lib.current_stream_ptr())
        if exact:
            self.ctx.check(self.L.vm_topk_cosine_seq_exact(*head, *tail))
        else:
            self.ctx.check(self.L.vm_topk_cosine_seq(*head, _ptr(self._counter(SeqScratch)), _ptr(scratch.flags),
                                                     *tail))
        _keep_alive(q, masks, idx)
        self._last[SeqScratch] = scratch
        return scores, rows, step_rows, step_scores

    def topk_seq(self, steps, k: int, max_step: int = 4, min_sep: Optional[int] = None, mask=None, mask_index=None,
                 max_gap_ms: Optional[int] = None, min_score: Optional[float] = None,
                 score_mode: int = _lib.VM_SCORE_RAW, exact: bool = False
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """-> (scores [C,k] float64, rows [C,k] int64, step_rows [C,k,J] int64, step_scores [C,k,J] float64): where each
        sequence of J <= 16 ORDERED steps - ``steps`` ``[C,J,D]`` or ``[J,D]``, frame or text embeddings - occurs in the
        memory, step j at most ``max_step`` <= 16 rows after step j-1.  ``rows`` are END row ids: the row of the last
        step of the best chain ``r_0 < ... < r_{J-1}`` ending there; ``step_rows`` is that chain and ``step_scores`` the
        reference cosine of each step with its row; ``scores`` their mean (summed left to right in fp64, bit for bit).

        Every row of a chain must be live and selected by ``mask`` (``mask`` / ``mask_index`` as in ``topk_masked``, one
        mask per sequence, default every live row); a chain may step over unselected rows.  On a tagged memory a chain
        stays within one video (no change of source between its first and last row; ``max_gap_ms``: no clock step
        backwards or above it between adjacent rows either).  Ties between predecessors go to the nearest row.  The k
        answers are PEAKS: end rows that rank before every other end row closer than ``min_sep`` rows (default
        ``min(32, (J-1) * max_step + 1)``) in (score desc, end row asc) - local-maximum suppression.  Score mapping and
        strict ``> min_score`` filter as in ``topk``; 0.0 / -1 / -1 / 0.0 padded.  ``J = 1, min_sep = 1`` is ``topk``
        (``topk_masked``); ``max_step = 1`` is ``topk_clip`` with its rows + J - 1.  Always the exhaustive answer: the fp32
        fast path redoes the sequences it cannot certify on the device, in the same call (csrc/topk_seq.hip).
        ``exact=True`` runs the exact layers over all rows (slow).  The per-sequence flags of the last call are in
        ``last_seq_flags``."""
        out = self.enqueue_topk_seq(steps, k, max_step=max_step, min_sep=min_sep, mask=mask, mask_index=mask_index,
                                    max_gap_ms=max_gap_ms, min_score=min_score, score_mode=score_mode, exact=exact)
        return tuple(t.clone() for t in out)

    # ---- range search (include/vidmem.h vm_range_cosine) ---------------------------------------------
    def prepare_range(self, Q: int, max_hits: int) -> "RangeScratch":
        """Size this memory's own range-search buffers for ``Q`` queries and ``max_hits`` hits each now (before a graph
        capture: a capture must not allocate)."""
        return self._resolve(RangeScratch, None, int(Q), int(max_hits))

    def _range_call(self, q: torch.Tensor, sc: Optional[torch.Tensor], min_score: float, score_mode: int,
                    max_hits: int, scratch: Optional["RangeScratch"], exact: bool) -> RangeHits:
        Q = q.shape[0]
        scratch = self._resolve(RangeScratch, scratch, Q, max_hits)
        rows = scratch.rows[:Q * max_hits].view(Q, max_hits)
        scores = scratch.scores[:Q * max_hits].view(Q, max_hits)
        lo, hi = (sc[0], sc[1]) if sc is not None else (None, None)
        head = (self.handle, _ptr(q), Q, float(min_score), int(score_mode), _ptr(lo), _ptr(hi), 1, 0, int(max_hits),
                _ptr(rows), _ptr(scores), _ptr(scratch.counts))
        tail = (_ptr(scratch.ws), scratch.ws.numel(), _lib.current_stream_ptr())
        if exact:
            self.ctx.check(self.L.vm_range_cosine_exact(*head, *tail))
        else:
            self.ctx.check(self.L.vm_range_cosine(*head, _ptr(scratch.rescored), *tail))
        _keep_alive(q, sc)
        self._last[RangeScratch] = scratch
        return RangeHits(scratch.counts[:Q], rows, scores)

    def _range_args(self, queries, min_score, scope, score_mode):
        ms = float(min_score)
        if math.isnan(ms):
            raise ValueError("the range threshold is NaN")
        if score_mode not in (_lib.VM_SCORE_RAW, _lib.VM_SCORE_UNIT_INTERVAL):
            raise ValueError("score_mode must be VM_SCORE_RAW or VM_SCORE_UNIT_INTERVAL")
        if scope is not None and not self.tagged:
            raise ValueError("a scope needs a tagged memory (EmbeddingMemory(..., tagged=True))")
        q = self._as_rows(queries)
        return q, (self._scopes(scope, q.shape[0]) if scope is not None else None), ms

    def enqueue_range(self, queries, min_score, scope=None, score_mode: int = _lib.VM_SCORE_RAW, max_hits: int = 1024,
                      scratch: Optional["RangeScratch"] = None) -> RangeHits:
        """The capturable range search -> ``RangeHits(counts, rows, scores)``: views of the buffers of ``scratch``
        (default: this memory's own, ``prepare_range``), valid until the next range call on it.

        Every row whose shown score is strictly above ``min_score``, in ascending row id (time order); the first
        ``max_hits`` of each query are written, ``counts`` holds the full number.  ``scope``: what ``topk_scoped`` takes
        (tagged memories; ``None`` = every live row, on any memory).  Enqueues ``vm_range_cosine`` on the current stream:
        nothing is read on the host.  Inside a graph capture pass ``scope`` as an int64 ``[Q, 2]`` device tensor
        (rewritten in place between replays) and a ``scratch`` the session owns, or call ``prepare_range`` first."""
        if int(max_hits) < 0:
            raise ValueError("max_hits is negative")
        q, sc, ms = self._range_args(queries, min_score, scope, score_mode)
        return self._range_call(q, sc, ms, score_mode, int(max_hits), scratch, False)

    def range_search(self, queries, min_score, scope=None, score_mode: int = _lib.VM_SCORE_RAW,
                     max_hits: Optional[int] = None, exact: bool = False) -> List[RangeResult]:
        """Every row above a threshold -> one ``RangeResult(rows, scores, count)`` per query: the rows (int64, ascending
        id = time order) whose shown score is strictly above ``min_score`` and their scores (float64, the reference's
        values bit for bit), on the device.  Always the exhaustive answer (include/vidmem.h vm_range_cosine).

        ``max_hits=None``: everything - a count-only call, ONE synchronising read of the counts, then the filling call
        with the exact size.  With a ``max_hits`` only the first ``max_hits`` hits of each query are returned and
        ``count`` still holds the query's full number, so a caller sees the truncation (one read of the counts too).
        ``scope``: as in ``topk_scoped``, tagged memories only; ``None`` = every live row, on any memory.
        ``exact=True`` scores every in-scope pair exactly instead of scanning first (slow; a checker).  The number of
        pairs the last fast call scored exactly is in ``last_range_rescored``."""
        q, sc, ms = self._range_args(queries, min_score, scope, score_mode)
        Q = q.shape[0]
        if max_hits is not None and int(max_hits) < 0:
            raise ValueError("max_hits is negative")
        if max_hits is None:
            counts = self._range_call(q, sc, ms, score_mode, 0, None, exact).counts.cpu().tolist()   # the one wait
            width = max(counts) if counts else 0
            if width == 0:
                return [RangeResult(torch.zeros(0, dtype=torch.int64, device=self.device),
                                    torch.zeros(0, dtype=torch.float64, device=self.device), 0) for _ in range(Q)]
            hits = self._range_call(q, sc, ms, score_mode, width, None, exact)
        else:
            hits = self._range_call(q, sc, ms, score_mode, int(max_hits), None, exact)
            counts = hits.counts.cpu().tolist()
        out = []
        for i, c in enumerate(counts):
            n = min(int(c), hits.rows.shape[1])
            out.append(RangeResult(hits.rows[i, :n].clone(), hits.scores[i, :n].clone(), int(c)))
        return out

    def moments(self, queries, min_score, scope=None, max_gap_ms: int = 1000,
                score_mode: int = _lib.VM_SCORE_RAW) -> List[List[Moment]]:
        """``range_search`` then ``segment_moments``: per query the runs of hits of one video that lie at most
        ``max_gap_ms`` apart, each with its first and last milliseconds and its peak - "one hit per event", ordered by
        (peak score descending, first row ascending).  Tagged memories only; the hits' tags are gathered on the device
        and read back once."""
        if not self.tagged:
            raise ValueError("moments needs a tagged memory (EmbeddingMemory(..., tagged=True))")
        found = self.range_search(queries, min_score, scope=scope, score_mode=score_mode)
        sizes = [int(f.rows.numel()) for f in found]
        if sum(sizes) == 0:
            return [[] for _ in found]
        col = _tensor_from_ptr(self.L.vm_memory_tags(self.handle), (self.capacity,), torch.int64, self.device)
        all_rows = torch.cat([f.rows for f in found])
        packed = torch.stack([all_rows, col[self._slots_of(all_rows)],
                              torch.cat([f.scores for f in found]).view(torch.int64)]).cpu().numpy()
        out, at = [], 0
        for n in sizes:
            part = packed[:, at:at + n]
            out.append(segment_moments(part[0], part[2].copy().view("float64"), part[1], max_gap_ms))
            at += n
        return out

    # ---- event segmentation (include/vidmem.h vm_memory_events / vm_memory_regroup_events) -----------
    def prepare_events(self, max_events: int = 0) -> "EventsScratch":
        """Size this memory's own event buffers for ``max_events`` first rows now (before a graph capture: a capture
        must not allocate)."""
        return self._resolve(EventsScratch, None, int(max_events))

    def _events_args(self, threshold, max_gap_ms, regroup: bool = False) -> Tuple[float, int]:
        """The argument rules of both calls, checked on the host before anything reaches the library."""
        if regroup and not self.grouped:
            raise ValueError("regroup_events needs a grouped memory (EmbeddingMemory(..., grouped=True))")
        tau = float(threshold)
        if math.isnan(tau):
            raise ValueError("the event threshold is NaN")
        gap = -1 if max_gap_ms is None else int(max_gap_ms)
        if gap >= 0 and not self.tagged:
            raise ValueError("max_gap_ms needs a tagged memory (EmbeddingMemory(..., tagged=True))")
        return tau, (gap if gap >= 0 else -1)

    def enqueue_events(self, threshold, max_gap_ms: Optional[int] = None, max_events: int = 1024,
                       with_links: bool = False, scratch: Optional["EventsScratch"] = None) -> EventsOut:
        """The capturable event segmentation -> ``EventsOut(count, first_rows, event_of, links)``: views of the buffers
        of ``scratch`` (default: this memory's own, ``prepare_events``), valid until the next events call on it.

        A row opens an event when it is the oldest live row, when its link - the reference cosine against the row
        before it - is not strictly above ``threshold``, or, on a tagged memory, when the source changes, exactly one
        of the two rows is untimed, or (``max_gap_ms`` given) the milliseconds step backwards or by more than
        ``max_gap_ms``.  Enqueues ``vm_memory_events`` on the current stream: nothing is read on the host."""
        tau, gap = self._events_args(threshold, max_gap_ms)
        max_events = int(max_events)
        if max_events < 0:
            raise ValueError("max_events is negative")
        scratch = self._resolve(EventsScratch, scratch, max_events)
        first = scratch.first_rows[:max_events]
        links = scratch.links if with_links else None
        self.ctx.check(self.L.vm_memory_events(self.handle, tau, gap, _ptr(links), _ptr(scratch.event_of), max_events,
                                               _ptr(first), _ptr(scratch.count), _ptr(scratch.ws), scratch.ws.numel(),
                                               _lib.current_stream_ptr()))
        return EventsOut(scratch.count, first, scratch.event_of, links)

    def events(self, threshold, max_gap_ms: Optional[int] = None, max_events: Optional[int] = None,
               with_links: bool = False) -> Events:
        """Cut the stored rows into events -> ``Events(first_rows, event_of, count, links)`` on the device, trimmed to
        what was written (``enqueue_events`` for the rule; ``segment_events`` turns the result into a list).

        ``max_events=None``: every event - the call is sized for the live row count, the most events there can be.
        With a ``max_events`` only the first ``max_events`` first rows are returned and ``count`` still holds the total.
        This form SYNCHRONISES once (it reads the count); the host row count must be current (``sync()``).  Two videos
        appended in alternation cut each other's events at every switch, and links chain: a slow pan is one event
        however far it drifts."""
        self._events_args(threshold, max_gap_ms)
        if max_events is not None and int(max_events) < 0:
            raise ValueError("max_events is negative")
        n = self.searchable
        width = n if max_events is None else int(max_events)
        out = self.enqueue_events(threshold, max_gap_ms, width, with_links)
        count = int(out.count.item()) if n else 0           # the one wait; an empty memory writes the count only
        return Events(out.first_rows[:min(count, width)].clone(), out.event_of[:n].clone(), count,
                      out.links[:n].clone() if with_links else None)

    def enqueue_regroup_events(self, threshold, max_gap_ms: Optional[int] = None, from_row=None,
                               scratch: Optional["EventsScratch"] = None) -> torch.Tensor:
        """The capturable regroup -> the device int64 [1] count of events opened among the rows it covered (a buffer of
        ``scratch``, default this memory's own).  Rewrites the group key and ordinal columns of a grouped memory so that
        every event is one group: key = the row id of the event's first row.  ``from_row=None``: the whole memory;
        an int or a device int64 [1] tensor (not read on the host): the rows from that id on - the row is judged against
        its predecessor and continues that row's group when it does not open an event.  Plain appends, each followed
        by a tail regroup from its first new row, leave what one whole regroup leaves, on a linear memory or a ring
        that has not wrapped and with no erase in between.  Afterwards the last event is closed: a later keyed append
        opens a new group whatever its key.  Enqueues ``vm_memory_regroup_events``: nothing is read on the host."""
        tau, gap = self._events_args(threshold, max_gap_ms, regroup=True)
        scratch = self._resolve(EventsScratch, scratch, 0)
        frm = None if from_row is None else self._int64_cell(from_row)
        self.ctx.check(self.L.vm_memory_regroup_events(self.handle, tau, gap, _ptr(frm), _ptr(scratch.count),
                                                       _ptr(scratch.ws), scratch.ws.numel(), _lib.current_stream_ptr()))
        _keep_alive(frm)
        self._last_keys_dev = None        # the keys are row ids now; the last event is closed on the device
        return scratch.count

    def regroup_events(self, threshold, max_gap_ms: Optional[int] = None, from_row=None) -> int:
        """``enqueue_regroup_events`` and one synchronising read -> the number of events among the covered rows."""
        return int(self.enqueue_regroup_events(threshold, max_gap_ms, from_row).item())

    # ---- group summaries (include/vidmem.h vm_memory_summaries) --------------------------------------
    def prepare_summaries(self, max_groups: int) -> "SummaryScratch":
        """Size this memory's own summary buffers for windows of ``max_groups`` groups now (before a graph capture: a
        capture must not allocate)."""
        max_groups = self._summary_args(0, max_groups)[1]
        return self._resolve(SummaryScratch, None, max_groups)

    def _summary_args(self, first_group, max_groups) -> Tuple[int, int]:
        """The argument rules of the summary calls, checked on the host before anything reaches the library."""
        if not self.grouped:
            raise ValueError("summaries need a grouped memory (EmbeddingMemory(..., grouped=True))")
        max_groups = int(max_groups)
        if max_groups < 0:
            raise ValueError("max_groups is negative")
        if isinstance(first_group, torch.Tensor):
            return first_group, max_groups
        first_group = int(first_group)
        if first_group < 0:
            raise ValueError("first_group is negative")
        return first_group, max_groups

    def enqueue_summaries(self, first_group=0, max_groups: int = 1024, key_frames: bool = True,
                          scratch: Optional["SummaryScratch"] = None) -> SummariesOut:
        """The capturable group summaries -> ``SummariesOut``: views of the buffers of ``scratch`` (default: this
        memory's own, ``prepare_summaries``), valid until the next summaries call on it.

        Window slot i holds live group ``first_group + i`` (groups are numbered in row order, the oldest live group is
        0): its first row id, row count, group key, centroid - the normalised fp64 mean of its rows, rounded once to
        the memory's dtype - and, with ``key_frames``, the stored row closest to that centroid and its RAW cosine.
        ``first_group``: an int, or a device int64 [1] tensor (not read on the host, so a captured graph can page).
        Enqueues ``vm_memory_summaries`` on the current stream: nothing is read on the host."""
        first_group, max_groups = self._summary_args(first_group, max_groups)
        scratch = self._resolve(SummaryScratch, scratch, max_groups)
        frm = self._int64_cell(first_group)
        m = max_groups
        out = SummariesOut(scratch.count, scratch.first_rows[:m], scratch.n_rows[:m], scratch.keys[:m],
                           scratch.centroids[:m], scratch.key_rows[:m] if key_frames else None,
                           scratch.key_scores[:m] if key_frames else None)
        # max_groups == 0: the count only - the empty views give null pointers
        self.ctx.check(self.L.vm_memory_summaries(self.handle, _ptr(frm), m, _ptr(out.centroids), _ptr(out.first_rows),
                                                  _ptr(out.n_rows), _ptr(out.keys), _ptr(out.key_rows),
                                                  _ptr(out.key_scores), _ptr(scratch.count), _ptr(scratch.ws),
                                                  scratch.ws.numel(), _lib.current_stream_ptr()))
        _keep_alive(frm)
        return out

    def summaries(self, first_group: int = 0, max_groups: Optional[int] = None) -> Summaries:
        """One centroid row and one key frame per group -> ``Summaries(first_rows, n_rows, keys, centroids, key_rows,
        key_scores, count)`` on the device, trimmed to the groups that were written (``enqueue_summaries`` for the
        rule).  ``max_groups=None``: every group from ``first_group`` on - a count-only call, then one sized call.
        ``count`` is always the total number of live groups.  This form SYNCHRONISES (it reads the count)."""
        first_group, _ = self._summary_args(first_group, 0 if max_groups is None else max_groups)
        if isinstance(first_group, torch.Tensor):
            raise ValueError("summaries() takes first_group as an int; enqueue_summaries accepts a device tensor")
        if max_groups is None:
            total = int(self.enqueue_summaries(first_group, 0).count.item())
            max_groups = max(total - first_group, 0)
        out = self.enqueue_summaries(first_group, int(max_groups))
        count = int(out.count.item())
        m = max(0, min(count - first_group, int(max_groups)))
        return Summaries(out.first_rows[:m].clone(), out.n_rows[:m].clone(), out.keys[:m].clone(),
                         out.centroids[:m].clone(), out.key_rows[:m].clone(), out.key_scores[:m].clone(), count)

    def consolidate(self, into: "EmbeddingMemory", first_group: int = 0, max_groups: Optional[int] = None
                    ) -> Tuple[Summaries, int]:
        """Append the centroids of the groups ``first_group ..`` to ``into``, a memory of the same ``dim`` and dtype ->
        ``(Summaries, first row id in into)``.  A centroid carries the tag of its key row when both memories are
        tagged and the source group's key when ``into`` is grouped; in ``into``'s id / meta tables it gets the id of
        the key row and ``{"first_row", "last_row", "key_row", "key_score"}``.  Paging: a second call with
        ``first_group`` = the first call's ``count`` adds only the groups that opened since (the last group of the
        first call may still have been growing: consolidate closed groups, or erase and redo the last summary)."""
        if not isinstance(into, EmbeddingMemory):
            raise ValueError("consolidate needs an EmbeddingMemory to append to")
        if into.dim != self.dim or into.dtype_name != self.dtype_name:
            raise ValueError(f"consolidate: {self.dim} x {self.dtype_name} rows do not fit a memory of "
                             f"{into.dim} x {into.dtype_name}")
        s = self.summaries(first_group, max_groups)
        m = int(s.first_rows.numel())
        if m == 0:
            return s, len(into)
        first, nrow = s.first_rows.tolist(), s.n_rows.tolist()
        krow, kscore = s.key_rows.tolist(), s.key_scores.tolist()
        tag = None
        if self.tagged and into.tagged:
            tags = _tensor_from_ptr(self.L.vm_memory_tags(self.handle), (self.capacity,), torch.int64, self.device)
            tag = tags[self._slots_of(s.key_rows)]
        meta = [{"first_row": a, "last_row": a + c - 1, "key_row": k, "key_score": v}
                for a, c, k, v in zip(first, nrow, krow, kscore)]
        at = into.append(s.centroids, ids=[self.id_of(k) for k in krow], meta=meta,
                         group=s.keys if into.grouped else None, tag=tag)
        return s, at

    # ---- what the last call of a kind left, and what its fast path could not certify -------------------------------
    last_flags = _last_property(TopkScratch, "flags", "int32 per query (vm_topk_flag): why the last fast `topk` call "
                                "redid a query exhaustively, 0 = certified")
    last_group_flags = _last_property(GroupedTopkScratch, "flags", "int32 per query (vm_topk_flag): why the last fast "
                                      "`topk_grouped` call redid a query, 0 = certified")
    last_scope_flags = _last_property(ScopedTopkScratch, "flags", "int32 per query (vm_topk_flag): why the last fast "
                                      "`topk_scoped` call redid a query, 0 = certified")
    last_group_scope_flags = _last_property(GroupedScopedTopkScratch, "flags", "int32 per query (vm_topk_flag): why the "
                                            "last fast `topk_grouped_scoped` call redid a query, 0 = certified")
    last_clip_flags = _last_property(ClipScratch, "flags", "int32 per clip (vm_topk_flag): why the last fast clip call "
                                     "redid a clip, 0 = certified")
    last_seq_flags = _last_property(SeqScratch, "flags", "int32 per sequence (vm_topk_flag): why the last fast sequence "
                                    "call redid a sequence, 0 = certified")
    last_range_rescored = _last_property(RangeScratch, "rescored", "int64 per query: the pairs the last fast range call "
                                         "scored exactly")
    last_mask_flags = _last_property(MaskedTopkScratch, "flags", "int32 per query (vm_topk_flag): why the last fast masked "
                                     "call redid a query, 0 = certified")
    masked_uncertified_count = _count_property(MaskedTopkScratch, "Queries the masked fast path")
    last_span_flags = _last_property(SpanTopkScratch, "flags", "int32 per query (vm_topk_flag): why the last fast "
                                     "`topk_span` call redid a query, 0 = certified")
    span_uncertified_count = _count_property(SpanTopkScratch, "Queries the span fast path")
    last_mix_flags = _last_property(MixTopkScratch, "flags", "int32 per mixed query (vm_topk_flag): why the last fast "
                                    "`topk_mix` call redid a query, 0 = certified")
    mix_uncertified_count = _count_property(MixTopkScratch, "Mixed queries the mixed fast path")
    last_fold_flags = _last_property(FoldTopkScratch, "flags", "int32 per fold query (vm_topk_flag): why the last fast "
                                     "`topk_fold` call redid a query, 0 = certified")
    fold_uncertified_count = _count_property(FoldTopkScratch, "Fold queries the any/all fast path")
    last_bias_flags = _last_property(BiasTopkScratch, "flags", "int32 per query (vm_topk_flag): why the last fast "
                                     "`topk_biased` call redid a query, 0 = certified")
    bias_uncertified_count = _count_property(BiasTopkScratch, "Queries the biased fast path")
    last_diverse_flags = _last_property(DiverseTopkScratch, "flags", "int32 per query (vm_topk_flag): why the pool stage "
                                        "of the last fast `topk_diverse` call redid a query, 0 = certified")
    diverse_uncertified_count = _count_property(DiverseTopkScratch, "Queries the diverse search's pool stage")
    grouped_uncertified_count = _count_property(GroupedTopkScratch, "Queries the grouped fast path")
    scoped_uncertified_count = _count_property(ScopedTopkScratch, "Queries the scoped fast path")
    group_scoped_uncertified_count = _count_property(GroupedScopedTopkScratch, "Queries the scoped grouped fast path")
    clip_uncertified_count = _count_property(ClipScratch, "Clips the clip search's fast path")
    seq_uncertified_count = _count_property(SeqScratch, "Sequences the sequence search's fast path")

    @property
    def uncertified_count(self) -> int:
        """Queries redone exhaustively since ``reset_uncertified`` on this memory's own top-k scratch."""
        own = self._own.get(TopkScratch)
        return 0 if own is None else int(own.uncert.item())

    def reset_uncertified(self) -> None:
        own = self._own.get(TopkScratch)
        if own is not None:
            own.uncert.zero_()

    def cosine_exact(self, queries, rows, as_f32: bool = False) -> torch.Tensor:
        """All-pairs reference cosine [Q,S] float64 between two row sets (neither needs to be stored).
        ``as_f32``: score the vectors as fp32 values instead of rounding them to the memory's 16-bit type first - what
        the post-compression filter uses, because its operands are fresh embedder outputs that never enter the
        memory and the reference compares the un-rounded floats with the threshold (retriever_hybrid.py:497-499)."""
        if as_f32:
            def f32(x):
                t = x if isinstance(x, torch.Tensor) else torch.tensor(x, dtype=torch.float32)
                if t.dim() == 1:
                    t = t.unsqueeze(0)
                return t.to(device=self.device, dtype=torch.float32).contiguous()
            q, r = f32(queries), f32(rows)
            if q.shape[-1] != r.shape[-1]:
                raise ValueError(f"embedding dimensions differ: {q.shape[-1]} vs {r.shape[-1]}")
            dim, dt = q.shape[-1], _lib.VM_F32
        else:
            q, r = self._as_rows(queries), self._as_rows(rows)
            dim, dt = self.dim, _lib.DTYPES[self.dtype_name]
        out = torch.empty((q.shape[0], r.shape[0]), dtype=torch.float64, device=self.device)
        self.ctx.check(self.L.vm_cosine_exact(self.ctx.handle, C.c_void_p(q.data_ptr()), q.shape[0],
                                              C.c_void_p(r.data_ptr()), r.shape[0], dim, dt,
                                              C.c_void_p(out.data_ptr()), _lib.current_stream_ptr()))
        _keep_alive(q, r)
        return out

    # ---- persistence: the reference's only durable store is the `embedding` list property
    # (src/components/neo4j_handler.py:229-242) and the export JSON (src/components/graph_exporter.py:61-67);
    # here: raw 16-bit rows in row-id order + the host id / meta tables, one .npz ------------------------------
    def _in_row_order(self, column: torch.Tensor) -> torch.Tensor:
        """A per-slot column over the searchable rows -> the same in row-id order: a ring that has wrapped keeps its
        oldest row at slot ``total % capacity``."""
        total = len(self)
        if not (self.ring and total > self.capacity):
            return column
        head = total % self.capacity
        return torch.cat([column[head:], column[:head]])

    def _slots_of(self, rows: torch.Tensor) -> torch.Tensor:
        """Row ids -> the slots that hold them, on every memory: a ring wraps, and elsewhere ids stay below capacity."""
        return rows % self.capacity

    def rows_host(self):
        """(first_row_id, uint16 [n, D]): the searchable rows as raw 16-bit patterns in row-id order (host copy)."""
        import numpy as np
        phys = self._in_row_order(self.rows_tensor().view(torch.int16))
        return len(self) - phys.shape[0], phys.cpu().numpy().view(np.uint16)

    def group_keys_host(self):
        """int64 [n]: the group key of every searchable row in row-id order (grouped memories; host copy)."""
        import numpy as np
        if not self.grouped:
            raise ValueError("not a grouped memory")
        keys = _tensor_from_ptr(self.L.vm_memory_group_keys(self.handle), (self.searchable,), torch.int64, self.device)
        return self._in_row_order(keys).cpu().numpy().astype(np.int64)

    def tags_host(self):
        """int64 [n]: the tag of every searchable row in row-id order (tagged memories; host copy)."""
        import numpy as np
        if not self.tagged:
            raise ValueError("not a tagged memory")
        tags = _tensor_from_ptr(self.L.vm_memory_tags(self.handle), (self.searchable,), torch.int64, self.device)
        return self._in_row_order(tags).cpu().numpy().astype(np.int64)

    def snapshot(self, path: str) -> None:
        import json
        import numpy as np
        base, rows = self.rows_host()
        total = base + rows.shape[0]
        extra = {"group_keys": self.group_keys_host()} if self.grouped else {}  # optional field: old files have none
        if self.tagged:
            extra["tags"] = self.tags_host()  # optional too: files without it restore untagged
        np.savez(path, rows=rows, dtype=self.dtype_name, dim=self.dim,
                 first_row_id=base, graph_uuid=self.graph_uuid or "",
                 ids=json.dumps([self.id_of(r) for r in range(base, total)]),
                 meta=json.dumps([self.meta_of(r) for r in range(base, total)]), **extra)

    @classmethod
    def restore(cls, path: str, capacity: Optional[int] = None, ring: bool = False, device: int = 0
                ) -> "EmbeddingMemory":
        """Row ids restart at 0 in the restored memory (ids / meta tables are restored in the same order).  A snapshot
        of a grouped memory restores grouped, with its key column (a group cut by a ring's window keeps its rows); one
        of a tagged memory restores tagged, with its tags."""
        import json
        import numpy as np
        z = np.load(path, allow_pickle=False)
        rows = torch.from_numpy(z["rows"].view(np.int16))
        dtype = str(z["dtype"])
        keys = z["group_keys"] if "group_keys" in z.files else None
        tags = z["tags"] if "tags" in z.files else None
        tagged_kw = {} if tags is None else {"tagged": True}
        mem = cls(capacity or max(rows.shape[0], 1), int(z["dim"]), dtype, ring=ring, device=device,
                  graph_uuid=str(z["graph_uuid"]) or None, grouped=keys is not None, **tagged_kw)
        if rows.shape[0]:
            group = None if keys is None else torch.from_numpy(keys.astype(np.int64))
            tag_kw = {} if tags is None else {"tag": torch.from_numpy(tags.astype(np.int64))}
            mem.append(rows.view(_torch_dtype(dtype)), ids=json.loads(str(z["ids"])), meta=json.loads(str(z["meta"])),
                       group=group, **tag_kw)
            if tags is not None and tags.size:  # sources handed out after a restore do not collide with stored ones
                real = tags[tags >= 0]
                mem._next_source = int(real.max() >> TAG_MS_BITS) + 1 if real.size else 0
            if keys is not None and keys.size:
                mem._next_group_key = max(0, int(keys.max()) + 1)
        return mem

    def _table_index(self, row: int) -> int:
        """The table slot of a LIVE row id, -1 for any other: a row a ring has overwritten has no entry any more, also
        while its slot has not been trimmed yet (``_trim_tables`` drops them late, in batches)."""
        if self.ring and row < len(self) - self.capacity:
            return -1
        return row - self.table_base

    def id_of(self, row: int) -> Optional[str]:
        i = self._table_index(row)
        return self.ids[i] if 0 <= i < len(self.ids) else None

    def meta_of(self, row: int) -> Optional[dict]:
        i = self._table_index(row)
        return self.meta[i] if 0 <= i < len(self.meta) else None


def topk_select(ctx: "_lib.Context", scores: torch.Tensor, k: int, col_limit: Optional[torch.Tensor] = None,
                row_base: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """[Q,S] fp64 all-pairs scores -> the k best columns of every row by (score descending, column ascending), query q
    ranking only columns < col_limit[q] (vm_topk_select; csrc/topk_exact.hip).  Rows = row_base + column, -1 padded."""
    Q, S = scores.shape
    scores = scores.contiguous()
    lim = None
    if col_limit is not None:
        lim = col_limit.to(device=scores.device, dtype=torch.int64).contiguous()
        if lim.shape != (Q,):
            raise ValueError("col_limit must hold one limit per query")
    out_s = torch.empty((Q, k), dtype=torch.float64, device=scores.device)
    out_r = torch.empty((Q, k), dtype=torch.int64, device=scores.device)
    ctx.check(ctx.L.vm_topk_select(ctx.handle, C.c_void_p(scores.data_ptr()), Q, S,
                                   C.c_void_p(lim.data_ptr() if lim is not None else 0), int(k), int(row_base),
                                   C.c_void_p(out_s.data_ptr()), C.c_void_p(out_r.data_ptr()),
                                   _lib.current_stream_ptr()))
    return out_s, out_r


def topk_merge(ctx: "_lib.Context", scores: torch.Tensor, rows: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[parts,Q,k] per-shard results -> global [Q,k] (csrc/topk.hip topk_merge_kernel)."""
    parts, Q, k = scores.shape
    scores = scores.contiguous()
    rows = rows.contiguous()
    out_s = torch.empty((Q, k), dtype=torch.float64, device=scores.device)
    out_r = torch.empty((Q, k), dtype=torch.int64, device=scores.device)
    ctx.check(ctx.L.vm_topk_merge(ctx.handle, C.c_void_p(scores.data_ptr()), C.c_void_p(rows.data_ptr()), parts, Q,
                                  k, C.c_void_p(out_s.data_ptr()), C.c_void_p(out_r.data_ptr()),
                                  _lib.current_stream_ptr()))
    return out_s, out_r


def _tensor_from_ptr(ptr: int, shape, dtype, device) -> torch.Tensor:
    """Wrap a raw device pointer owned by libvidmem as a torch tensor (no copy, no ownership)."""
    import numpy as np

    class _Holder:
        pass

    n = 1
    for s in shape:
        n *= s
    itemsize = torch.empty(0, dtype=dtype).element_size()
    h = _Holder()
    h.__cuda_array_interface__ = {
        "shape": (n * itemsize,), "typestr": "|u1", "data": (int(ptr), False), "version": 3, "strides": None,
    }
    raw = torch.as_tensor(h, device=device)
    return raw.view(dtype).view(*shape)
