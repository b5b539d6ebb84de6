"""CPU: the lifecycle harness (tests/lifecycle_ref.py) proved before it judges a kernel.

1. the model against itself: provenance, two erases = one erase of the union, restored() = a fresh model of the window;
2. the conditions both scripts must meet at every checkpoint, for both dtypes, from the reference alone - those of the
   nine older readers, and that the probes of the five newer ones (``topk_masked``, ``topk_span``, ``topk_mix``,
   ``topk_diverse``, ``recall_links``, fed by ``mask_of_rows`` / ``mask_of_scope`` / ``mask_where``) are not vacuous: the
   masks select some and not all, a stale mask is not a remapped one, dead slots lie under the all-ones mask after a
   reset, the ring cuts a span, W and lam change a ranking, ``exclude_group`` changes a link; and those of the three newest
   (``topk_biased`` with ``bias_of_rows`` / ``bias_of_age``, ``topk_fold``, ``topk_seq``): the boost and the age column
   change a ranking, a stale column is not a remapped one, in the wrapped ring the column by slot is not the column by
   row - base, dead slots lie under the fill, max and min rank different rows, the sequence across a change of source
   loses to its untagged self, the masked sequence ends where the unmasked one does over another chain, and in the
   wrapped ring a chain has rows on both sides of the physical wrap;
3. planted defects: a fake memory answers ``checkpoint`` from a second model instance, all seventeen readers, the mask and
   the column builders in numpy; the unplanted fake passes, every defect planted in that instance fails with its reader's
   name.
"""
import weakref
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import cref
from tests import bias_ref as BR
from tests import clip_ref as CL
from tests import diverse_ref as DR
from tests import erase_ref as E
from tests import events_ref as V
from tests import fold_ref as FR
from tests import group_ref as G
from tests import lifecycle_ref as LC
from tests import mask_ref as MR
from tests import mix_ref as XR
from tests import scope_ref as S
from tests import seq_ref as SQ
from tests import span_ref as SP

DTYPES = ["f16", "bf16"]
SCRIPTS = {"linear": (LC.linear_script, 1600, False), "ring": (LC.ring_script, 600, True)}


class Refused(Exception):
    code = LC.VM_ERR_UNSUPPORTED


def _norms(bits, dtype):
    return np.linalg.norm(CL.from_bits(np.ascontiguousarray(bits), dtype).astype(np.float64), axis=1)


class _Mask(np.ndarray):
    """A row mask of the fake memory: int32 words, so that ``~ & |`` work as on the device tensor.  Every one made is
    remembered weakly: the defect "mask_remapped" has to find the masks a caller kept."""
    made = []

    def __array_finalize__(self, obj):
        _Mask.made = [r for r in _Mask.made if r() is not None] + [weakref.ref(self)]


class _Col(np.ndarray):
    """A bias column (or a stack of them) of the fake memory, remembered weakly as the masks are: the defect
    "bias_remapped" has to find the columns a caller kept."""
    made = []

    def __array_finalize__(self, obj):
        _Col.made = [r for r in _Col.made if r() is not None] + [weakref.ref(self)]


STALE_NORMS = ("stale_norm", "mix_stale_norm", "diverse_stale_norm", "bias_stale_norm", "fold_stale_norm")


class FakeMemory:
    """The surface of ``EmbeddingMemory`` that the scripts and ``checkpoint`` use, answered from a ``Model`` of its own.
    ``defect`` plants one way a real memory could go wrong."""

    def __init__(self, model: LC.Model, defect=None):
        self.m, self.defect = model, defect
        self.W = MR.mask_words(model.capacity)
        self.slots = np.zeros((model.capacity, model.D), np.uint16)    # the rows of a linear memory that never zeroes a
                                   # slot: what lies under the bits beyond the live count (defect "mask_sees_dead_slots")
        self.old_ids = None        # the ids before the last erase (defect "where_ids_stale")
        self.last_diverse_mmr = None   # of the last topk_diverse call
        self.ghost = None          # rows an erase left in the slots it vacated (defect "ghost")
        self.stale = None          # the norms an erase left behind in slots [0, n') (defect "stale_norm")
        self.memo = {}             # reader answers since the last mutation: checkpoint asks for both forms of each
        self.join = None           # the live index where the last erase made two rows adjacent (defect "seq_spans_sources")

    # -- accessors
    def __len__(self):
        return self.m.total

    @property
    def searchable(self):
        return self.m.total - self.m.base

    def rows_host(self):
        lo, live = self.m.window()
        return lo + (self.defect == "ring_base" and self.m.wrapped), live.rows

    def tags_host(self):
        return self.m.window()[1].tags

    def group_keys_host(self):
        return self.m.window()[1].keys

    def id_of(self, r):
        return self.m.ids[r] if self.m.base <= r < self.m.total else None

    def raw(self, n):
        _, live = self.m.window()
        out = []
        for col in (live.rows, live.tags, live.keys, live.ords):
            full = np.zeros((n,) + col.shape[1:], col.dtype)
            full[:col.shape[0]] = col
            out.append(full)
        if self.ghost is not None:
            k = live.rows.shape[0]
            out[0][k:k + self.ghost.shape[0]] = self.ghost[:n - k]
        return out

    # -- mutators
    def meta_of(self, r):
        return None if self.id_of(r) is None else {"i": self.id_of(r)}

    def _sync(self):
        """The live rows into their slots; whatever lay behind them stays."""
        if not self.m.ring:
            self.slots[:self.m.total] = self.m.rows

    def append(self, rows, ids=None, meta=None, group=None, tag=None):
        self.ghost = self.old_ids = None
        first = self.m.append(rows, tag, group, ids)
        self._sync()
        return first

    def append_novel(self, rows, tau, ids=None, meta=None, group=None, tag=None):
        known = None
        if self.ghost is not None:                          # the search sees the rows that were not zeroed
            lo, live = self.m.window()
            known = LC.N.top1(rows, np.concatenate([live.rows, self.ghost]), self.m.dtype, base=lo)
        n_ids = len(self.m.ids)
        keep, row_of = self.m.append_novel(rows, tau, tag, group, ids, known=known)
        if self.defect == "gated_ids":                      # the first ids of the batch, not the kept rows' ids
            self.m.ids = self.m.ids[:n_ids] + list(ids)[:int(keep.sum())]
        self.ghost = self.old_ids = None
        self._sync()
        return SimpleNamespace(keep=keep, row_of=row_of, kept=int(keep.sum()))

    def erase(self, rows=None, scope=None):
        m = self.m
        old = SimpleNamespace(rows=m.rows, tags=m.tags, ords=m.ords, ids=m.ids)
        out = m.erase_rows(rows) if rows is not None else m.erase_scopes(scope)
        if out is None:
            raise Refused("erase: the ring has wrapped")
        n, keep = m.total, out.new_row_of >= 0
        if self.defect in STALE_NORMS and out.count:
            self.stale = _norms(old.rows[:n], m.dtype)
        if self.defect == "where_ids_stale":
            self.old_ids = old.ids
        if self.defect == "mask_remapped":                  # every mask anybody holds follows its rows
            seen = set()
            for ref in _Mask.made:
                mask = ref()
                if mask is None or mask.shape != (self.W,) or mask.__array_interface__["data"][0] in seen:
                    continue
                seen.add(mask.__array_interface__["data"][0])
                was = np.nonzero(MR.selected(np.array(mask).view(np.uint32), 0, keep.size, m.capacity))[0]
                mask[...] = MR.pack_rows(out.new_row_of[was][keep[was]], m.capacity).view(np.int32)
        if self.defect == "bias_remapped":                  # every column anybody holds follows its rows
            seen = set()
            for ref in _Col.made:
                col = ref()
                if col is None or col.shape != (BR.bias_stride(m.capacity),) or col.__array_interface__["data"][0] in seen:
                    continue
                seen.add(col.__array_interface__["data"][0])
                was = np.array(col)
                col[...] = 0
                col[out.new_row_of[keep]] = was[np.nonzero(keep)[0]]
        gone = np.nonzero(~keep)[0]
        if gone.size and keep[gone[0]:].any():
            self.join = int(out.new_row_of[gone[0] + np.nonzero(keep[gone[0]:])[0][0]])
        self._sync()
        if self.defect == "tags_not_moved":
            m.tags = old.tags[:n]
        if self.defect == "ordinals_not_rederived":
            m.ords = old.ords[keep]
        if self.defect == "ghost":
            self.ghost = old.rows[n:]
        if self.defect == "ids_not_remapped":
            m.ids = old.ids[:n]
        return SimpleNamespace(count=out.count, new_row_of=out.new_row_of)

    def regroup_events(self, threshold, max_gap_ms=None, from_row=None):
        m = self.m
        if from_row is None:
            return m.regroup_whole(threshold, max_gap_ms)
        if self.defect == "wrong_side" and m.wrapped and from_row % m.capacity == 0 and m.base < from_row < m.total:
            # the predecessor of the row in slot 0 is read from the slot on the other side of the wrap - the oldest live
            # row, which does not resemble it: the row opens an event where it should continue one.  The count it reports
            # is the right one, so that only what the call left in the columns gives it away
            lo, flags = m.flags(threshold, max_gap_ms)
            count = int(flags[from_row - lo:].sum())
            flags[from_row - lo] = True
            out = V.regroup_tail(m.keys[lo:], m.ords[lo:], flags, from_row - lo, lo)
            m.keys, m.ords = np.concatenate([m.keys[:lo], out.keys]), np.concatenate([m.ords[:lo], out.ordinals])
            m.state = out.state
            return count
        return m.regroup_tail(threshold, max_gap_ms, from_row)

    def reset(self):
        last = self.m.state[1]
        self.m.reset()
        self.ghost = self.stale = self.old_ids = self.join = None
        if self.defect == "reset_keeps_open":
            self.m.state = (0, last, 1)

    # -- readers
    def _once(self, fn, *args):
        """``fn(*args)``, computed once while the model stands still (every mutation moves the total or the state)."""
        key = (fn.__name__, self.m.total, self.m.state, self.stale is None) + tuple(
            a.tobytes() if isinstance(a, np.ndarray) else repr(a) for a in args)
        if key not in self.memo:
            self.memo = {k: v for k, v in self.memo.items() if k[1:3] == key[1:3]}
            self.memo[key] = fn(*args)
        return self.memo[key]

    def topk(self, q, k, min_score=None, exact=False):
        return self._once(self._topk, q, k, min_score)

    def _topk(self, q, k, min_score):
        lo, live = self.m.window()
        if self.defect == "stale_norm" and self.stale is not None and live.rows.shape[0]:
            scale = self._stale_scale()                     # scores from the norms the erase left behind
            scores = cref.cosine_matrix(np.ascontiguousarray(q), np.ascontiguousarray(live.rows), dtype=self.m.dtype) * scale
            r, s = S.scoped_topk_from_scores(scores, live.tags, LC.SCOPE_ALL, k, min_score=min_score, base=lo)
            return s, r
        if min_score is not None:
            r, s = cref.cosine_topk(np.ascontiguousarray(q), np.ascontiguousarray(live.rows), k, dtype=self.m.dtype,
                                    min_score=min_score)
            return s, np.where(r >= 0, r + lo, -1)
        r, s = self.m.exp_topk(q, k)
        return s, r

    def topk_grouped(self, q, k, exact=False):
        r, s, kk = self._once(self.m.exp_grouped, q, k)
        return s, r, kk

    def topk_scoped(self, q, k, scope, exact=False):
        r, s = self._once(self.m.exp_scoped, q, scope, k)
        return s, r

    def topk_grouped_scoped(self, q, k, scope, exact=False):
        r, s, kk = self._once(self.m.exp_grouped_scoped, q, scope, k)
        return s, r, kk

    def topk_clip(self, clips, k, exact=False):
        r, s = self._once(self.m.exp_clip, clips, k)
        return s, r

    def range_search(self, q, min_score, scope=None, max_hits=None, exact=False):
        return [SimpleNamespace(rows=r[:max_hits], scores=s[:max_hits], count=c)
                for r, s, c in self._once(self.m.exp_range, q, min_score, scope)]

    def events(self, threshold, max_gap_ms=None, with_links=False):
        link, seg = self._once(self.m.exp_events, threshold, max_gap_ms)
        return SimpleNamespace(first_rows=seg.first_rows, event_of=seg.event_of, count=seg.count, links=link)

    def summaries(self):
        s = self._once(self.m.exp_summaries)
        return SimpleNamespace(count=int(s.first_rows.size), **s._asdict())

    def _stale_scale(self):
        """Per live row: its norm over the norm the erase left in its slot."""
        _, live = self.m.window()
        scale = np.ones(live.rows.shape[0])
        n = min(self.stale.size, scale.size)
        scale[:n] = _norms(live.rows[:n], self.m.dtype) / np.where(self.stale[:n] > 0, self.stale[:n], 1.0)
        return scale

    # -- masks: int32 words [W] as on the device
    def _mask(self, ids):
        return MR.pack_rows(ids, self.m.capacity).view(np.int32).view(_Mask)

    def new_mask(self, n=1):
        return np.zeros((n, self.W), np.int32).view(_Mask)

    def mask_of_rows(self, rows):
        ids = np.asarray(rows, np.int64).ravel()
        return self._mask(ids[(ids >= self.m.base) & (ids < self.m.total)])

    def mask_of_scope(self, scope):
        lo, live = self.m.window()
        return self._mask(lo + np.nonzero(E.mask_of_scopes(live.tags, scope))[0])

    def mask_where(self, fn):
        ids = self.m.ids if self.old_ids is None else self.old_ids      # defect "where_ids_stale": the ids before the erase
        return self._mask([r for r in range(self.m.base, self.m.total) if fn(r, ids[r], {"i": ids[r]})])

    def _selection(self, mask, mask_index, Q):
        lo, live = self.m.window()
        words = np.array(mask).view(np.uint32).reshape(-1, self.W)
        return MR.selection(words, mask_index, Q, lo, live.rows.shape[0], self.m.capacity)

    def rows_of_mask(self, mask):
        return (self.m.base + np.nonzero(self._selection(mask, None, 1)[0])[0]).tolist()

    # -- the readers whose operands speak about row ids and slots
    def topk_masked(self, q, k, mask, mask_index=None, exact=False):
        return self._once(self._topk_masked, q, k, np.array(mask), mask_index)

    def _topk_masked(self, q, k, mask, mask_index):
        lo, live = self.m.window()
        rows, sel = live.rows, self._selection(mask, mask_index, q.shape[0])
        n, hi = rows.shape[0], self.m.written
        if self.defect == "mask_sees_dead_slots" and not self.m.ring and hi > n:   # bits past the live count count too
            rows = self.slots[:hi]
            sel = MR.selection(mask.view(np.uint32).reshape(-1, self.W), mask_index, q.shape[0], 0, hi, self.m.capacity)
        r, s = MR.masked_topk(q, rows, sel, k, dtype=self.m.dtype, base=lo)
        return s, r

    def topk_span(self, q, k, span, exact=False):
        pairs = [tuple(int(x) for x in p) for p in span] if isinstance(span, np.ndarray) else list(span)
        return self._once(self._topk_span, q, k, SP.pairs(pairs, q.shape[0]))

    def _topk_span(self, q, k, pairs):
        lo, live = self.m.window()
        if self.defect == "span_by_slot" and self.m.wrapped:                # the bounds compared with the slot
            slot = (lo + np.arange(live.rows.shape[0])) % self.m.capacity
            sel = np.stack([(slot >= a) & (slot <= b) for a, b in pairs])
            r, s = MR.masked_topk(q, live.rows, sel, k, dtype=self.m.dtype, base=lo)
        else:
            r, s = self.m.exp_span(q, pairs, k)
        return s, r

    def topk_mix(self, terms, weights, k, mask=None, mask_index=None, exact=False):
        return self._once(self._topk_mix, terms, weights, k, None if mask is None else np.array(mask), mask_index)

    def _topk_mix(self, terms, weights, k, mask, mask_index):
        lo, live = self.m.window()
        sel = None if mask is None else self._selection(mask, mask_index, terms.shape[0])
        scores = XR.mix_scores_loop
        if self.defect == "mix_stale_norm" and self.stale is not None and live.rows.shape[0]:
            scale = self._stale_scale()
            scores = lambda e, w: XR.mix_scores_loop(e * scale, w)
        r, s = XR.mix_topk(terms, weights, live.rows, sel, k, dtype=self.m.dtype, base=lo, scores=scores)
        return s, r

    def topk_diverse(self, q, k, pool=None, lam=0.5, mask=None, mask_index=None, exact=False):
        s, r, self.last_diverse_mmr = self._once(self._topk_diverse, q, k, pool, np.asarray(lam), np.array(mask), mask_index)
        return s, r

    def _topk_diverse(self, q, k, pool, lam, mask, mask_index):
        lo, live = self.m.window()
        sim = None
        if self.defect == "diverse_stale_norm" and self.stale is not None and live.rows.shape[0]:
            scale = self._stale_scale()
            sim = DR.sim_matrix(live.rows, self.m.dtype) * scale[:, None] * scale[None, :]
        r, s, v = DR.diverse_topk(q, live.rows, self._selection(mask, mask_index, q.shape[0]), k, pool, list(lam),
                                  dtype=self.m.dtype, base=lo, sim=sim)
        return s, r, v

    def _aged(self):
        """A wrapped ring, or a linear memory after an erase: where the defects that need no stale operand are planted, so
        that the script gets going before they show."""
        return self.m.wrapped or self.m.total < self.m.used

    def recall_links(self, first_row, n_rows, k=10, min_gap=1, max_back=None, exclude_group=False, block=256, exact=False):
        aged = self._aged()                                                 # the links go wrong on an aged memory only:
        own = exclude_group and not (aged and self.defect == "links_own_group")     # a wrapped ring, or after an erase
        r, s = self._once(self.m.exp_links, first_row, n_rows, k, min_gap, max_back, own)
        done = n_rows // block * block
        if aged and self.defect == "links_page_edge" and done < n_rows:     # the last, ragged page is never searched
            r, s = r.copy(), s.copy()
            r[done:], s[done:] = -1, 0.0
        return s, r

    # -- bias columns: fp32 [S] by slot as on the device
    def new_bias(self, n=1):
        return np.zeros((n, BR.bias_stride(self.m.capacity)), np.float32).view(_Col)

    def bias_of_rows(self, rows, values, out=None, clear=True):
        lo, live = self.m.window()
        col = self.new_bias()[0] if out is None else out
        col[...] = BR.bias_from_rows_ref(np.asarray(rows, np.int64).ravel(), values, lo, live.rows.shape[0], self.m.capacity,
                                         start=None if clear else col)
        return col

    def bias_of_age(self, now_ms, per_ms, fill=0.0, out=None):
        lo, live = self.m.window()
        col = self.new_bias()[0] if out is None else out
        col[...] = BR.bias_from_tags_ref(live.tags, lo, self.m.capacity, now_ms, per_ms, fill)
        return col

    def topk_biased(self, q, k, bias, weight=None, bias_index=None, mask=None, mask_index=None, exact=False):
        return self._once(self._topk_biased, q, k, np.array(bias), tuple(weight), tuple(bias_index),
                          None if mask is None else np.array(mask), mask_index)

    def _topk_biased(self, q, k, bias, weight, bias_index, mask, mask_index):
        m = self.m
        lo, live = m.window()
        rows, Q = live.rows, q.shape[0]
        n, hi = rows.shape[0], m.written
        sel = None if mask is None else self._selection(mask, mask_index, Q)
        b = BR.row_bias(bias, list(bias_index), Q, lo, n, m.capacity)
        if self.defect == "bias_by_row" and m.wrapped:      # the entry at row - base, not at the slot
            b = BR.row_bias(bias, list(bias_index), Q, 0, n, m.capacity)
        if self.defect == "bias_sees_dead_slots" and not m.ring and hi > n:      # the slots past the live count rank too
            rows, b = self.slots[:hi], BR.row_bias(bias, list(bias_index), Q, 0, hi, m.capacity)
            sel = None if mask is None else MR.selection(mask.view(np.uint32).reshape(-1, self.W), mask_index, Q, 0, hi, m.capacity)
        e = cref.cosine_matrix(np.ascontiguousarray(q), np.ascontiguousarray(rows), dtype=m.dtype) if rows.shape[0] else np.zeros((Q, 0))
        if self.defect == "bias_stale_norm" and self.stale is not None and n:
            e = e * self._stale_scale()
        r, s = BR.bias_topk_from_cosines(e, list(weight), b, sel, k, base=lo)
        return s, r

    def topk_fold(self, terms, k, op="max", weights=None, mask=None, mask_index=None, exact=False):
        return self._once(self._topk_fold, terms, k, op, weights, None if mask is None else np.array(mask), mask_index)

    def _topk_fold(self, terms, k, op, weights, mask, mask_index):
        lo, live = self.m.window()
        sel = None if mask is None else self._selection(mask, mask_index, terms.shape[0])
        scores = FR.fold_scores_loop
        if self.defect == "fold_stale_norm" and self.stale is not None and live.rows.shape[0]:
            scale = self._stale_scale()
            scores = lambda e, w, o: FR.fold_scores_loop(e * scale, w, o)
        if self.defect == "fold_term_of_max" and op == "min" and self._aged():      # the right score, the other op's term
            scores = lambda e, w, o: (FR.fold_scores_loop(e, w, "min")[0], FR.fold_scores_loop(e, w, "max")[1])
        weights = [[1.0] * terms.shape[1]] * terms.shape[0] if weights is None else weights
        r, s, t = FR.fold_topk(terms, weights, live.rows, sel, k, op, dtype=self.m.dtype, base=lo, scores=scores)
        return s, r, t

    def topk_seq(self, steps, k, max_step=4, min_sep=None, mask=None, mask_index=None, max_gap_ms=None, exact=False):
        return self._once(self._topk_seq, steps, k, max_step, min_sep, None if mask is None else np.array(mask), mask_index,
                          max_gap_ms)

    def _topk_seq(self, steps, k, G, min_sep, mask, mask_index, max_gap_ms):
        m = self.m
        lo, live = m.window()
        C, J, n = steps.shape[0], steps.shape[1], live.rows.shape[0]
        out = (np.zeros((C, k)), np.full((C, k), -1, np.int64), np.full((C, k, J), -1, np.int64), np.zeros((C, k, J)))
        if n == 0:
            return out
        el = SQ.eligible(n, C, None if mask is None else self._selection(mask, mask_index, C))
        brk = CL.tag_breaks(live.tags, -1 if max_gap_ms is None else max_gap_ms)
        w = (-lo) % m.capacity                              # the live index of the row in slot 0
        if self.defect == "seq_wrong_side" and m.wrapped and 0 < w < n:
            brk[w] = True       # its predecessors are read from the other side of the wrap: no chain continues into slot 0
        if self.defect == "seq_spans_sources" and self.join is not None and self.join < n:
            brk[self.join] = False                          # the break between the two rows an erase made adjacent
        for c in range(C):
            b = brk | ~el[c] if self.defect == "seq_mask_blocks" and self._aged() else brk     # an unselected row ends a chain
            r, s, sr, ss = SQ.from_scores(CL.frame_scores(steps[c], live.rows, m.dtype), el[c], b, k, G, min_sep, base=lo)
            out[0][c], out[1][c], out[2][c], out[3][c] = s, r, sr, ss
        return out

    last_mask_flags = last_span_flags = last_mix_flags = last_diverse_flags = np.zeros(6, np.int32)
    last_bias_flags = last_fold_flags = last_seq_flags = np.zeros(6, np.int32)
    bias_uncertified_count = fold_uncertified_count = seq_uncertified_count = 0
    uncertified_count = grouped_uncertified_count = scoped_uncertified_count = 0
    group_scoped_uncertified_count = clip_uncertified_count = 0
    masked_uncertified_count = span_uncertified_count = mix_uncertified_count = diverse_uncertified_count = 0


class FakeIO:
    """What ``checkpoint`` needs beside the memory's surface, for the fake."""
    t = staticmethod(lambda bits: np.asarray(bits))
    i64 = staticmethod(lambda x: np.asarray(x, np.int64))
    bits = staticmethod(lambda x: np.asarray(x))
    stack = staticmethod(lambda masks: np.stack([np.asarray(m) for m in masks]))
    f64 = staticmethod(lambda x: np.asarray(x, np.float64))
    i64d = staticmethod(lambda x: np.asarray(x, np.int64))
    col_at = staticmethod(lambda col, slots: np.asarray(col)[slots])
    keep = staticmethod(lambda col: col.copy())
    ordinals = staticmethod(lambda mem: mem.m.window()[1].ords)
    raw = staticmethod(lambda mem, n: mem.raw(n))
    restore = staticmethod(lambda mem, capacity: FakeMemory(mem.m.restored(capacity), mem.defect))


def _driver(script, dtype, defect=None, hooks=()):
    _, cap, ring = SCRIPTS[script]
    D = LC.DIMS[dtype]
    return LC.Driver(FakeMemory(LC.Model(D, dtype, cap, ring), defect), LC.Model(D, dtype, cap, ring), FakeIO, hooks)


# ---- 1. the model against itself -------------------------------------------------------------------------------------
def _filled(dtype="f16", n=300, capacity=400, ring=False):
    bits, scene = LC.pool(dtype)
    m = LC.Model(LC.DIMS[dtype], dtype, capacity, ring)
    m.append(bits[:n], [LC.make_tag(i // 120, (i % 120) * LC.MS) for i in range(n)], 10_000 + scene[:n] % 5,
             [f"r{i}" for i in range(n)], np.arange(n))
    return m, bits


def _state(m):
    return (m.rows.tobytes(), m.tags.tolist(), m.keys.tolist(), m.ords.tolist(), m.ids, m.prov.tolist(), m.state)


def test_two_erases_equal_one_erase_of_the_union():
    a, _ = _filled()
    b, _ = _filled()
    first = a.erase_scopes([(LC.make_tag(1, 10 * LC.MS), LC.make_tag(1, 70 * LC.MS))])
    second = a.erase_rows([0, 5, 140, 141, 200, -1, 999])
    old_ids = np.nonzero(first.new_row_of >= 0)[0][[0, 5, 140, 141, 200]]
    union = E.mask_of_scopes(b.tags, [(LC.make_tag(1, 10 * LC.MS), LC.make_tag(1, 70 * LC.MS))]) | E.mask_of_rows(300, old_ids)
    once = b._erase(union)
    assert first.count == 61 and second.count == 5 and once.count == 66
    assert np.array_equal(E.compose(first.new_row_of, second.new_row_of), once.new_row_of)
    assert _state(a) == _state(b)
    assert a.used == 300 and a.total == 234 and a.state[2] == 1 and a.ords[-1] + 1 == a.state[0]


def test_restored_equals_a_fresh_model_of_the_window():
    for ring, cap in ((False, 400), (True, 256)):
        m, bits = _filled(capacity=cap, ring=ring)
        m.regroup_whole(LC.THRESHOLD, LC.GAP_MS)
        lo, live = m.window()
        assert lo == (44 if ring else 0)
        fresh = LC.Model(m.D, m.dtype, 400)
        fresh.append(live.rows, live.tags, live.keys, live.ids, live.prov)
        back = m.restored(400)
        assert _state(back) == _state(fresh) and back.state == (int(G.group_ids(live.keys)[-1]) + 1, int(live.keys[-1]), 1)
        assert np.array_equal(back.ords, G.group_ids(live.keys)) and back.ids[0] == f"r{lo}"
        assert np.array_equal(back.rows, bits[back.prov])


def test_append_follows_the_open_group_rule_and_reset_forgets_it():
    m, bits = _filled(n=20)
    last = int(m.keys[-1])
    groups = m.state[0]
    m.append(bits[20:23], [0, 1, 2], [last, last, 7], ["a", "b", "c"])         # continues, then opens
    assert m.ords[-3:].tolist() == [groups - 1, groups - 1, groups] and m.state == (groups + 1, 7, 1)
    m.regroup_whole(2.0, -1)                                                    # every row its own event; closed
    assert m.state == (23, 22, 0) and m.keys.tolist() == list(range(23))
    m.append(bits[23:24], [3], [22], ["d"])                                     # the closed group's key opens a group
    assert m.ords[-1] == 23 and m.state == (24, 22, 1)
    m.reset()
    m.append(bits[:2], [0, 1], [22, 22], ["e", "f"])
    assert m.ords.tolist() == [0, 0] and m.state == (1, 22, 1) and m.total == 2 and m.used == 2


# ---- 2. the conditions of the scripts ----------------------------------------------------------------------------------
ONCE = ("stale mask differs from a remapped one", "W ranks other rows than term 0", "a lam < 1 query leaves its pool's first k",
        "a link row with an empty past, or live rows before the window", "exclude_group changes a link",
        "the flag-0 demand is made of every reader",
        # the biased, the any/all and the sequence search
        "the boost column changes a query's rows", "the age column changes a query's rows",
        "a stale bias column selects other rows than a remapped one", "max and min rank different rows",
        "sequence (d) scores lower on the tagged window than without tags",
        "sequence (e) ends at the same row under its mask, over another chain",
        "the flag-0 demand is made of topk_biased", "the flag-0 demand is made of topk_fold",
        "the flag-0 demand is made of topk_seq")
ONCE_WRAPPED = ("the bias column read by slot is not the column read by row - base",
                "sequence (c) has step rows on both sides of the physical wrap")
OLDER = ("masked", "masked2", "span", "span_carried", "mix", "mix_masked", "diverse")     # the readers ``must_certify`` had
DEAD_SLOTS = ("5 erase scope", "6 erase top-k rows, whole regroup", "9 empty", "9 append after erase-to-empty",
              "10 reset, append", "2 erase scope", "8 reset, append")


def _new_reader_conditions(label, d, p, exp, once, at):
    """The probes of the masked, span, mixed and diverse searches and of the recall links are not vacuous: from the
    oracle's values alone.  ``once`` counts what has to hold at least once per script."""
    m = d.model
    lo, live = m.window()
    n, k, total = live.rows.shape[0], p.k, m.total
    sels, sel = [r.size for r in exp["mask_rows"]], exp["sel"]
    if n == 0:
        assert all(c == 0 for c in sels) and not sel.any(), at
        newer = ("biased", "biased_masked", *(LC.fold_name(*c) for c in LC.FOLD_CALLS), *LC.SEQ_CALLS, "seq_one")
        for name in ("masked", "masked2", "span", "mix", "mix_masked", "diverse", *newer):
            assert (exp[name][0] == -1).all() and not exp[name][1].any(), at + name
            assert all((x == -1).all() if x.dtype.kind == "i" else not x.any() for x in exp[name][2:]), at + name
        assert (exp["bias_cols"][2] == np.float32(LC.AGE_FILL)).all(), at + "bias_of_age of the empty memory is not all fill"
        assert not exp["diverse"][2].any() and all(r.shape == (0, LC.LINK_K) for r, _ in exp["links"]), at
        assert not any(any(v) for v in exp["must_certify"].values()), at
        return
    # masks (b), (c), (d): each selects at least k rows, so its query's answer is full, and not every live row ((b), one
    # source and a window, only where two sources are live); among the six queries at least one has k selected rows and at
    # least one (the empty mask) fewer
    sources = np.unique(live.tags >> LC.MS_BITS).size
    assert sels[0] == n and all(k <= c < n + (i == 0 and sources == 1) for i, c in enumerate(sels[1:4])), \
        at + f"the masks select {sels} of {n} rows, {sources} sources"
    per_query = sel.sum(axis=1)
    assert (per_query >= k).any() and (per_query < k).any(), at + f"rows selected per query {per_query.tolist()}"
    assert (exp["masked"][0][:4] >= 0).all() and (exp["masked"][0][5] == -1).all(), at
    if d.last_erase is not None and p.carried is not None:      # stale: the bit names whichever row lives in the slot now
        new = d.last_erase
        for words, stale in zip(p.carried, exp["mask_rows"][4:]):
            was = np.nonzero(MR.selected(words, 0, new.size, m.capacity))[0]
            remapped = np.sort(new[was][new[was] >= 0])
            once["stale mask differs from a remapped one"] += not np.array_equal(remapped, stale)
    if label in ("9 append after erase-to-empty", "10 reset, append", "8 reset, append"):
        assert m.written > n, at + "no slot beyond the live count was ever written: the all-ones mask covers nothing dead"
    # spans
    span_rows = exp["span"][0]
    assert np.array_equal(span_rows[0], exp["topk"][0][0]), at + "the open span is not topk"
    assert (span_rows[4] == -1).all() and span_rows[5].tolist() == [total - 1] + [-1] * (k - 1), at
    assert (span_rows[1] <= lo + n // 2).all() and (span_rows[2][span_rows[2] >= 0] <= lo + 20).all(), at
    assert sorted(span_rows[3][span_rows[3] >= 0]) == list(range(max(lo, total - 3), total)), at
    if m.wrapped:           # ids lo - 5 .. lo - 1 named rows once; the ring has overwritten them: the span is cut by base
        assert lo - 5 >= 0 and p.spans[2][0] == lo - 5 < lo and (span_rows[2] >= lo).all(), at
        by_slot = [r for r in range(lo, total) if p.spans[2][0] <= r % m.capacity <= p.spans[2][1]]
        assert by_slot != list(range(lo, lo + 21)), at + "the span by slots is the span by row ids"
    # mixed, diverse, links
    once["W ranks other rows than term 0"] += any(not np.array_equal(exp["mix"][0][c], exp["topk"][0][c]) for c in range(1, 6))
    once["a lam < 1 query leaves its pool's first k"] += any(
        set(exp["diverse"][0][i]) != set(exp["masked"][0][i]) for i in range(1, 5))
    assert all(set(exp["diverse"][0][i]) - {-1} <= set(m.exp_masked(p.queries, sel, LC.POOL)[0][i]) for i in range(6)), at
    first, count = p.links
    assert count == min(n, LC.LINK_ROWS) and first + count == total and first >= lo, at
    once["a link row with an empty past, or live rows before the window"] += bool(
        (exp["links"][0][0] == -1).all(axis=1).any() or first > lo)
    plain = m.exp_links(first, count, LC.LINK_K, LC.LINK_GAP, None, False)
    once["exclude_group changes a link"] += not np.array_equal(plain[0], exp["links"][0][0])
    must = exp["must_certify"]
    assert not (must["masked"][5] or must["mix_masked"][5] or must["diverse"][5] or must["span"][4]), at + "an empty query"
    if m.outside:
        assert not any(any(v) for v in must.values()), at + "the sticky word is set: every query goes to the redo"
    once["the flag-0 demand is made of every reader"] += all(any(v) for name, v in must.items() if name in OLDER)
    _newest_reader_conditions(label, d, p, exp, once, at)


def _newest_reader_conditions(label, d, p, exp, once, at):
    """The probes of the biased, the any/all and the sequence search are not vacuous, from the oracle's values alone."""
    m = d.model
    lo, live = m.window()
    n, k, cap = live.rows.shape[0], p.k, m.capacity
    q, cols, index, W = p.queries, exp["bias_cols"], list(LC.BIAS_INDEX), list(LC.BIAS_W)
    once["the boost column changes a query's rows"] += not np.array_equal(exp["biased"][0][1], exp["topk"][0][1])
    once["the age column changes a query's rows"] += not np.array_equal(exp["biased"][0][2], exp["topk"][0][2])
    if d.last_erase is not None and p.carried_bias is not None:     # stale: the entry names whichever row lives in the slot now
        new = d.last_erase
        kept = np.nonzero(new >= 0)[0]
        remapped = cols.copy()
        remapped[3] = 0
        remapped[3][new[kept] % cap] = p.carried_bias[kept % cap]
        once["a stale bias column selects other rows than a remapped one"] += not np.array_equal(
            m.exp_biased(q, remapped, None, k)[0][3], exp["biased"][0][3])
    slots = (lo + np.arange(n)) % cap
    dead = np.setdiff1d(np.arange(cols.shape[1]), slots)
    assert (cols[2][dead] == np.float32(LC.AGE_FILL)).all() and (np.abs(cols[2][slots]) < 2.0 ** 40).all(), at
    assert np.abs(LC.AGE_FILL * max(W)) > 2 + np.abs(cols[:, slots]).max() * max(np.abs(W)), at + "the fill would not win"
    if label in DEAD_SLOTS:         # a slot that held a row once and holds none now lies under the fill
        assert m.written > n and (cols[2][n:m.written] == np.float32(LC.AGE_FILL)).all(), at + "no dead slot under the fill"
    e = cref.cosine_matrix(np.ascontiguousarray(q), np.ascontiguousarray(live.rows), dtype=m.dtype)
    if m.wrapped:
        by_row = BR.bias_topk_from_cosines(e, W, BR.row_bias(cols, index, 6, 0, n, cap), None, k, base=lo)
        once[ONCE_WRAPPED[0]] += not np.array_equal(by_row[0], exp["biased"][0])
        step_slots = exp["seq"][2][2, 0] % cap
        once[ONCE_WRAPPED[1]] += bool(exp["seq"][0][2, 0] >= 0 and step_slots.max() >= cap - 3 and step_slots.min() <= 2)
    once["max and min rank different rows"] += not np.array_equal(exp["fold_max"][0], exp["fold_min"][0])
    assert all(((exp[LC.fold_name(*c)][2] >= 0) == (exp[LC.fold_name(*c)][0] >= 0)).all() for c in LC.FOLD_CALLS), at
    free = m.exp_seq(p.seqs[3:4], None, k, LC.SEQ_G, 1, tags=False)
    once["sequence (d) scores lower on the tagged window than without tags"] += bool(free[1][0, 0] > exp["seq"][1][3, 0])
    plain = m.exp_seq(p.seqs[4:5], None, k, LC.SEQ_G, LC.SEQ_CALLS["seq_masked"][0])
    under = exp["seq_masked"]
    assert p.seq_excluded not in under[2][4], at + "a chain of sequence (e) holds the row its mask leaves out"
    once["sequence (e) ends at the same row under its mask, over another chain"] += bool(
        under[0][4, 0] == plain[0][0, 0] >= 0 and not np.array_equal(under[2][4, 0], plain[2][0, 0]))
    must = exp["must_certify"]
    # as for the older readers: every named call of the reader is asked for flag 0 at one checkpoint
    once["the flag-0 demand is made of topk_biased"] += any(must["biased"]) and any(must["biased_masked"])
    once["the flag-0 demand is made of topk_fold"] += all(any(must[LC.fold_name(*c)]) for c in LC.FOLD_CALLS)
    once["the flag-0 demand is made of topk_seq"] += all(any(must[name]) for name in (*LC.SEQ_CALLS, "seq_one"))


def _conditions(seen, once=None):
    once = {} if once is None else once
    once.update({name: 0 for name in ONCE + ONCE_WRAPPED})

    def hook(label, d, p, exp):
        lo, live = d.model.window()
        n = live.rows.shape[0]
        at = f"[{d.dtype} {label}] "
        seen.append((label, n))
        _new_reader_conditions(label, d, p, exp, once, at)
        # provenance: every live row is, bit for bit, the row it came from
        assert (live.prov >= 0).all() and all(np.array_equal(live.rows[i], d.src[int(live.prov[i])]) for i in range(n)), at
        assert len(live.ids) == n and len(set(live.ids)) == n
        readers = [exp["topk"][0], exp["grouped"][0], exp["scoped"][0], exp["grouped_scoped"][0]]
        if n == 0:          # the empty memory: padding and zero counts everywhere
            assert all((r == -1).all() for r in readers) and all((c[0] == -1).all() for c in exp["clip"]), at
            assert all(c == 0 for _, _, c in exp["range"]) and exp["events"][1].count == 0, at
            assert exp["summaries"].first_rows.size == 0, at
            return
        # well-formed: the ordinals the device keeps are the runs of the keys, so the key-based oracles apply
        assert np.array_equal(live.ords - live.ords[0], G.group_ids(live.keys)), at + "ordinals are not the runs of the keys"
        assert (live.keys >= 0).all(), at + "a plain append's key"
        full = [i for i in range(6) if all((r[i] >= 0).all() for r in readers)]
        short = [i for i in range(6) if any((r[i] < 0).any() for r in readers)]
        assert len(full) >= 3 and short, at + f"queries with k hits everywhere {full}, with fewer {short}"
        for i, sc in enumerate(p.scopes):
            if sc[0] > sc[1]:                                # the empty scope: only padding
                assert (exp["scoped"][0][i] == -1).all() and (exp["grouped_scoped"][0][i] == -1).all(), at
                assert exp["range"][i][2] == 0, at
        counts = [c for _, _, c in exp["range"]]
        assert sum(counts) > 0 and max(counts) < p.max_hits, at + f"range counts {counts}"
        assert exp["events"][1].count > 1, at
        assert all((c[0][0] >= 0).any() for c in exp["clip"]), at + "a clip without a hit"
        if n % 16 == 0:
            raise AssertionError(at + "a multiple of 16 live rows")
        gone = d.gone is not None and not any(np.array_equal(d.src[d.gone], r) for r in live.rows)
        if gone:            # the row that was erased or gated away does not come back with score 1
            assert exp["topk"][1][3, 0] < 0.9999, at
    return hook


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_script_conditions_and_the_unplanted_fake(dtype):
    seen, once = [], {}
    d = _driver("linear", dtype, hooks=[_conditions(seen, once)])
    end = LC.linear_script(d)
    assert all(once[name] >= 1 for name in ONCE), once
    labels = [s[0] for s in seen]
    assert len(labels) == 13 and labels[0].startswith("1 ") and labels[-1].startswith("10 ")
    assert all(0.2 <= g <= 0.8 for g in d.gated) and len(d.gated) == 2, d.gated
    live = dict(seen)
    assert live["4 append source 1, tail regroup"] > 512 and live["7 append_novel into vacated slots"] > 512
    assert live["9 empty"] == 0 and max(live.values()) < 1600 and d.stored + end.stored < 1600
    assert end.model.state[2] == 1 and end.model.ords[0] == 0          # step 10 opened a group


@pytest.mark.parametrize("dtype", DTYPES)
def test_ring_script_conditions_and_the_unplanted_fake(dtype):
    seen = []

    def wrap_hook(label, d, p, exp):
        m = d.model
        if m.ring and m.total > 2 * m.capacity:
            lo, live = m.window()
            cap = m.capacity
            assert m.keys[2 * cap - 1] == m.keys[2 * cap], "no group spans slots capacity - 1 and 0"
            assert (2 * cap - 1) % cap == cap - 1 and (2 * cap) % cap == 0
            assert live.keys[0] < lo, "the first live group is not a cut one"
            # links_ref's group_of: the model's ordinals as they are and the runs of the keys cut the same spans, and a
            # row of the cut group has no past outside its group
            first, count = p.links
            by_ords = SP.link_spans(lo, m.total - lo, lo, LC.LINK_GAP, None, live.ords)
            assert by_ords == SP.link_spans(lo, m.total - lo, lo, LC.LINK_GAP, None, G.group_ids(live.keys))
            assert live.ords[1] == live.ords[0] and by_ords[1][1] == lo - 1
            assert by_ords[first - lo:] == SP.link_spans(first, count, lo, LC.LINK_GAP, None, live.ords)
            seen.append(("wrapped twice", lo))

    once = {}
    d = _driver("ring", dtype, hooks=[_conditions(seen, once), wrap_hook])
    LC.ring_script(d)
    assert all(once[name] >= 1 for name in ONCE + ONCE_WRAPPED), once
    labels = [s[0] for s in seen]
    assert labels.count("wrapped twice") == 2 and "7 restored linear" in labels and labels[-1] == "8 reset, append"
    assert all(0.2 <= g <= 0.8 for g in d.gated) and len(d.gated) == 1, d.gated
    assert d.stored < 1600


# ---- 3. planted defects ----------------------------------------------------------------------------------------------------
DEFECTS = [("stale_norm", "linear", "default topk"), ("tags_not_moved", "linear", "tags_host"),
           ("ghost", "linear", "past the live count"), ("ids_not_remapped", "linear", "id_of"),
           ("gated_ids", "linear", "id_of"), ("reset_keeps_open", "linear", "raw ordinals"),
           ("ordinals_not_rederived", "ring", "ordinals relative"), ("ring_base", "ring", "first live row"),
           ("wrong_side", "ring", "group_keys_host"),
           ("mask_sees_dead_slots", "linear", "topk_masked"), ("mask_remapped", "linear", "carried"),
           ("where_ids_stale", "linear", "mask_where"), ("span_by_slot", "ring", "topk_span"),
           ("mix_stale_norm", "linear", "topk_mix"), ("diverse_stale_norm", "linear", "last_diverse_mmr"),
           ("links_own_group", "linear", "recall_links max_back=None exclude_group=True"),
           ("links_page_edge", "ring", "recall_links"),
           ("bias_remapped", "linear", "topk_biased"), ("bias_by_row", "ring", "topk_biased"),
           ("bias_sees_dead_slots", "linear", "topk_biased"), ("bias_stale_norm", "linear", "topk_biased"),
           ("fold_stale_norm", "linear", "topk_fold"), ("fold_term_of_max", "linear", "term indices"),
           ("seq_wrong_side", "ring", "topk_seq"), ("seq_spans_sources", "linear", "topk_seq seq_gap"),
           ("seq_mask_blocks", "linear", "topk_seq seq_masked")]


@pytest.mark.parametrize("defect,script,message", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_planted_defect_fails_the_checkpoint(defect, script, message):
    d = _driver(script, "f16", defect)
    with pytest.raises(AssertionError) as e:
        SCRIPTS[script][0](d)
    assert message in str(e.value), str(e.value)[:300]
    assert d.log, "the defect showed before the first checkpoint passed: the script did not get going"


def test_fewer_live_rows_than_steps_is_padding():
    """No script checkpoint has between 1 and 3 live rows (below 16 the probes are never-stored rows and the window is
    empty), so the rule is held here directly: with fewer live rows than the sequence has steps there is no chain, and the
    model, the oracle's loop statement and the fake all return padding; with exactly J rows the one chain is the answer."""
    bits, _ = LC.pool("f16")
    for n in (1, LC.SEQ_J - 1, LC.SEQ_J):
        m, _ = _filled(n=n, capacity=8)
        steps = SQ.steps_at(bits, "f16", np.arange(LC.SEQ_J)[None], 3)
        want = m.exp_seq(steps, None, LC.K, LC.SEQ_G, 1)
        loop = SQ.seq_topk_loop(steps, m.rows, LC.K, LC.SEQ_G, 1, "f16", tags=m.tags)
        s, r, sr, ss = FakeMemory(m).topk_seq(steps, LC.K, max_step=LC.SEQ_G, min_sep=1)
        for got in (loop, (r, s, sr, ss)):
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), n
        if n < LC.SEQ_J:
            assert (want[0] == -1).all() and not want[1].any() and (want[2] == -1).all() and not want[3].any(), n
        else:
            assert want[0][0].tolist() == [n - 1] + [-1] * (LC.K - 1) and want[2][0, 0].tolist() == list(range(n))


def test_ghost_rows_are_seen_by_the_next_gated_append():
    """The vacated slot that was not zeroed: the next gated batch is suppressed by a row that no longer exists."""
    m, bits = _filled(n=60, capacity=100)
    fake = FakeMemory(m, "ghost")
    clean, _ = _filled(n=60, capacity=100)
    for mem in (fake, FakeMemory(clean)):
        mem.erase(rows=list(range(40, 60)))
    batch = LC.noisy(bits[55:58], "f16", 3, 0.02)
    tags, keys, ids = [LC.make_tag(2, i) for i in range(3)], [1, 2, 3], ["x", "y", "z"]
    got = fake.append_novel(batch, 0.99, ids=ids, group=keys, tag=tags)
    want = FakeMemory(clean).append_novel(batch, 0.99, ids=ids, group=keys, tag=tags)
    assert want.kept == 3 and got.kept == 0 and (got.row_of >= 40).all()
