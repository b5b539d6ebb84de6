"""One host model of the whole memory (include/vidmem.h), numpy only.

Every feature of the memory has its own oracle; this file composes them into ONE model that is carried through a whole
life - keyed, tagged and gated appends, erases, whole and tail regroups, the ring overwrite, reset, snapshot / restore -
and says after every step what all seventeen readers must return (torch only where the existing data generators use it,
``pool`` and ``noisy``).  The readers: ``topk``, ``topk_grouped``, ``topk_scoped``, ``topk_grouped_scoped``, ``topk_clip``,
``range_search``, ``events``, ``summaries``, each top-k one with an exact form, the five whose operands speak about row
ids and slots - ``topk_masked``, ``topk_span``, ``topk_mix``, ``topk_diverse`` (with ``last_diverse_mmr``) and
``recall_links`` - fed by the mask builders ``mask_of_rows``, ``mask_of_scope``, ``mask_where`` and read back through
``rows_of_mask``, and the three newest: ``topk_biased`` over columns built by ``bias_of_rows`` and ``bias_of_age`` (a
column speaks about physical slots, as a mask does), ``topk_fold`` (max and min, with its term indices) and ``topk_seq``
(which walks predecessors through the slots and applies the tag-break rule between adjacent rows).  It defines no cosine
and no ranking of its own: every
mutator restates the header's rule by calling the oracle that already states it (novelty_ref.gate, erase_ref.erase,
events_ref.regroup / regroup_tail), every expectation is the feature's own oracle over the live window (mask_ref,
span_ref, mix_ref, diverse_ref, bias_ref, fold_ref and seq_ref for the eight newer readers).

``Model``       the state, in row-id order, and the mutators.
``checkpoint``  compares an ``EmbeddingMemory`` (or anything with its surface) with the model through the public
                accessors and all seventeen readers, each top-k reader in its default and its ``exact`` form; bit equality.
                Where a feature's own oracle condition says that the fast path must certify a query of the masked, span,
                mixed, diverse, biased, any/all or sequence search, its flag of the default call must be 0: the redo may
                not hide a broken scan.
``Driver``      applies one step to the model and to the memory, compares what the step returns, builds the probes.
``linear_script`` / ``ring_script``  the two lives of tests/test_lifecycle_gpu.py; tests/test_lifecycle_cpu.py runs the
                same scripts against a fake memory, proves the conditions they must meet and plants defects.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from oracle import cref
from tests import bias_ref as BR
from tests import clip_ref as CL
from tests import diverse_ref as DR
from tests import erase_ref as E
from tests import events_ref as V
from tests import fold_ref as FR
from tests import group_ref as G
from tests import group_scope_ref as GS
from tests import mask_ref as MR
from tests import mix_ref as XR
from tests import novelty_ref as N
from tests import range_ref as R
from tests import scope_ref as S
from tests import seq_ref as SQ
from tests import span_ref as SP
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
MASK_INDEX = (0, 1, 2, 3, 4, -1)       # the mask of each probe query: (a) .. (d), the carried exclusion, -1 = the empty mask
MASK_INDEX2 = (5, 4, -1, 2, 1, 3)      # a second masked search: the carried complement, every query under another mask
WEIGHTS = [[1.0, 0.0, 0.0]] + [[1.0, 0.5, -0.25]] * 5         # the mixed queries: C = 6, J = 3
POOL, LAM = 16, (1.0, 0.5, 0.5, 0.3, 0.7, 0.0)                # the diverse search: k = 5 of a pool of 16
LINK_ROWS, LINK_K, LINK_GAP, LINK_BLOCK = 300, 3, 2, 128      # recall links of the newest 300 rows: pages of 128, 128, 44
LINK_CALLS = ((None, True), (200, False))                     # (max_back, exclude_group)
DOMAIN = (2.0 ** -40, 2.0 ** 40)       # the norms inside which the fp32 stage's bound holds (include/vidmem.h)
# the biased search: four columns - (0) zeros, (1) bias_of_rows of the rows topk just showed, (2) bias_of_age, (3) column
# (1) as the previous checkpoint built it, searched again, stale, after the mutation.  Query i reads column BIAS_INDEX[i]
# (9: out of range = the zero column) with weight BIAS_W[i] (bias_ref.BETAS: 0.0, a negative and a tiny one among them)
BIAS_INDEX = (0, 1, 2, 3, 9, 1)
BIAS_W = (BR.BETAS[0], BR.BETAS[2], BR.BETAS[3], BR.BETAS[0], BR.BETAS[4], BR.BETAS[1])
BIAS_PLAIN = (0, 4, 5)                 # the zero column, the index out of range, the weight 0.0: these queries are topk's
AGE_PER_MS, AGE_FILL = 1.0e-3, 1.0e6   # a frame (33 ms) of age costs 0.033 x the weight; the fill would win every ranking
FOLD_CALLS = tuple((op, w, m) for op in FR.OPS for w in (False, True) for m in (False, True))   # (op, WEIGHTS?, masks?)
SEQ_J, SEQ_G = 4, 3                    # the six sequences: four steps, at most three rows apart
SEQ_MASK_INDEX = (0, 1, 2, 3, 6, 4)    # (a) .. (d) under the checkpoint's masks (a) .. (d), (e) under its own mask (the
                                       # seventh: every row but the chain's second), (f) under the carried exclusion
# name -> (min_sep, max_gap_ms, masks?)
SEQ_CALLS = {"seq": (1, None, False), "seq_masked": (4, None, True), "seq_gap": (4, GAP_MS, False)}


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
    mask_scopes: list      # mask (b): two tag ranges, one source and a window, in one mask_of_scope call
    carried: tuple         # the model's words of the previous checkpoint's exclusion mask and of its complement, or None
    spans: list            # six (lo, hi) in row ids, None = open
    carried_span: tuple    # (lo + 10, total - 10) of the previous checkpoint, or None
    terms: np.ndarray      # uint16 [6, 3, D]: the mixed queries
    links: tuple           # (first_row, n_rows) of the recall links
    bias_now: int          # now_ms of bias_of_age: the newest live tag's clock
    carried_bias: object   # the model's column (1) of the previous checkpoint, fp32 [S] by slot, or None
    seqs: np.ndarray       # uint16 [6, 4, D]: the sequences (a) .. (f)
    seq_excluded: int      # the row id the mask of sequence (e) leaves out, -1 when there is none
    k: int = K
    max_hits: int = MAX_HITS
    threshold: float = THRESHOLD
    gap_ms: int = GAP_MS


class Model:
    """Rows, tags, keys, ordinals, ids and provenance of every row appended since the last reset or erase renumbering,
    in row-id order; ``state`` = (groups opened, last key, open); ``used`` = slots a linear memory has written since the
    last reset (an erase zeroes what it vacates, a reset promises nothing about the columns); ``written`` = slots written
    since the memory was created, which a reset does not forget: what may still lie under a mask bit or inside a span;
    ``outside`` = the sticky word of vm_memory_create: a row whose norm is neither 0 nor in [2^-40, 2^40] was appended
    since the last reset, so every search is answered by the exhaustive redo."""

    def __init__(self, D, dtype, capacity, ring=False):
        self.D, self.dtype, self.capacity, self.ring = int(D), dtype, int(capacity), bool(ring)
        self.written = 0
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
        self.outside = False

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
        self.written = max(self.written, min(self.total, self.capacity))
        self.outside = self.outside or not in_domain(rows, self.dtype).all()
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

    def exp_masked(self, q, sel, k):
        lo, live = self.window()
        return MR.masked_topk(q, live.rows, sel, k, dtype=self.dtype, base=lo)

    def exp_span(self, q, spans, k):
        lo, live = self.window()
        return SP.span_topk(q, live.rows, spans, k, dtype=self.dtype, base=lo)

    def exp_mix(self, terms, weights, sel, k):
        lo, live = self.window()
        return XR.mix_topk(terms, weights, live.rows, sel, k, dtype=self.dtype, base=lo)

    def exp_diverse(self, q, sel, k, pool, lam):
        lo, live = self.window()
        return DR.diverse_topk(q, live.rows, sel, k, pool, list(lam), dtype=self.dtype, base=lo)

    def exp_biased(self, q, cols, sel, k):
        """``cols`` fp32 [4, S] by slot; bias_ref.row_bias maps slots to rows: the header's rule - the entry names whichever
        row lives in the slot now."""
        lo, live = self.window()
        return BR.bias_topk(q, live.rows, cols, list(BIAS_INDEX), list(BIAS_W), sel, k, dtype=self.dtype, base=lo,
                            capacity=self.capacity)

    def exp_fold(self, terms, weights, sel, k, op):
        lo, live = self.window()
        return FR.fold_topk(terms, _fold_weights(weights, terms), live.rows, sel, k, op, dtype=self.dtype, base=lo)

    def exp_seq(self, steps, sel, k, G, min_sep, max_gap_ms=None, tags=True):
        lo, live = self.window()
        return SQ.seq_topk(steps, live.rows, k, G, min_sep, dtype=self.dtype, tags=live.tags if tags else None, sel=sel,
                           max_gap_ms=-1 if max_gap_ms is None else max_gap_ms, base=lo)

    def bias_columns(self, p: "Probes", shown):
        """fp32 [4, S] by slot, from the model alone: zeros, bias_ref.bias_from_rows_ref of the rows shown with
        ``boost_values``, bias_ref.bias_from_tags_ref, and the carried column as it was (zeros when there is none)."""
        lo, live = self.window()
        n, S = live.rows.shape[0], BR.bias_stride(self.capacity)
        shown = np.asarray(shown, np.int64).ravel()
        carried = np.zeros(S, np.float32) if p.carried_bias is None else p.carried_bias
        return np.stack([np.zeros(S, np.float32), BR.bias_from_rows_ref(shown, boost_values(shown), lo, n, self.capacity),
                         BR.bias_from_tags_ref(live.tags, lo, self.capacity, p.bias_now, AGE_PER_MS, AGE_FILL), carried])

    def exp_links(self, first, count, k, min_gap, max_back, exclude_group):
        """span_ref.links_ref wants ``group_of`` as the group of every live row in row order, indexed by r - base, and
        only compares neighbours: the model's ordinals as they are, a cut first group included."""
        lo, live = self.window()
        return _links(live.rows.tobytes(), live.ords.tobytes() if exclude_group else None, self.D, self.dtype, lo, k, first,
                      count, min_gap, max_back)

    def mask_selections(self, p: Probes, shown):
        """bool [6, n]: what the six masks of a checkpoint select among the live rows, from the model alone.  (a) all
        ones: every live row; (b) mask_of_scope: by the tags; (c) ~mask_of_rows(shown): the live rows that are not in
        ``shown``; (d) mask_where: by the ids; (e) the carried exclusion mask and its complement: the header's staleness
        rule - the bit names whichever row lives in the slot now (mask_ref.selected of the old words)."""
        lo, live = self.window()
        n = live.rows.shape[0]
        ids = lo + np.arange(n, dtype=np.int64)
        shown = np.asarray(shown, np.int64)
        sels = [np.ones(n, bool), E.mask_of_scopes(live.tags, p.mask_scopes).astype(bool).reshape(n),
                ~np.isin(ids, shown[shown >= 0]),
                np.array([where(lo + i, name, {"i": name}) for i, name in enumerate(live.ids)], bool).reshape(n)]
        for words in p.carried or (None, None):
            sels.append(np.zeros(n, bool) if words is None else MR.selected(words, lo, n, self.capacity))
        return np.stack(sels)

    def expect(self, p: Probes):
        lo, live = self.window()
        n = live.rows.shape[0]
        q, k = p.queries, p.k
        exp = {"topk": self.exp_topk(q, k), "grouped": self.exp_grouped(q, k),
               "scoped": self.exp_scoped(q, p.scopes, k),
               "grouped_scoped": self.exp_grouped_scoped(q, p.scopes, k),
               "clip": [self.exp_clip(c, k) for c in p.clips],
               "range": self.exp_range(q, p.range_min, p.scopes),
               "events": self.exp_events(p.threshold, p.gap_ms), "summaries": self.exp_summaries()}
        sels = self.mask_selections(p, exp["topk"][0])
        pick = lambda index: np.stack([sels[i] if 0 <= i < len(sels) else np.zeros(n, bool) for i in index])
        sel, sel2 = pick(MASK_INDEX), pick(MASK_INDEX2)
        span_sets = {"span": p.spans}
        if p.carried_span is not None:
            span_sets["span_carried"] = [p.carried_span] * 6
        exp["mask_rows"] = [lo + np.nonzero(s)[0] for s in sels]
        exp["sel"] = sel
        exp["masked"], exp["masked2"] = self.exp_masked(q, sel, k), self.exp_masked(q, sel2, k)
        for name, spans in span_sets.items():
            exp[name] = self.exp_span(q, spans, k)
        exp["mix"], exp["mix_masked"] = self.exp_mix(p.terms, WEIGHTS, None, k), self.exp_mix(p.terms, WEIGHTS, sel, k)
        exp["diverse"] = self.exp_diverse(q, sel, k, POOL, LAM)
        exp["links"] = [self.exp_links(*p.links, LINK_K, LINK_GAP, back, own) for back, own in LINK_CALLS]
        cols = exp["bias_cols"] = self.bias_columns(p, exp["topk"][0])
        exp["biased"], exp["biased_masked"] = self.exp_biased(q, cols, None, k), self.exp_biased(q, cols, sel, k)
        for op, w, m in FOLD_CALLS:
            exp[fold_name(op, w, m)] = self.exp_fold(p.terms, WEIGHTS if w else None, sel if m else None, op=op, k=k)
        ids = lo + np.arange(n, dtype=np.int64)
        seq_sel = exp["seq_sel"] = np.stack([np.concatenate([sels, (ids != p.seq_excluded)[None]])[i] for i in SEQ_MASK_INDEX])
        for name, (sep, gap, m) in SEQ_CALLS.items():
            exp[name] = self.exp_seq(p.seqs, seq_sel if m else None, k, SEQ_G, sep, gap)
        exp["seq_one"] = self.exp_seq(q[:, None, :], None, k, SEQ_G, 1)
        # where the fast path must certify: each feature's own condition, on the oracle's scores (never on the device's)
        new = ("biased", "biased_masked", *(fold_name(*c) for c in FOLD_CALLS), *SEQ_CALLS, "seq_one")
        must = {name: [False] * 6 for name in ("masked", "masked2", "mix", "mix_masked", "diverse", *span_sets, *new)}
        if n and not self.outside:
            sc = cref.cosine_matrix(np.ascontiguousarray(q), np.ascontiguousarray(live.rows), dtype=self.dtype)
            e = cref.cosine_matrix(np.ascontiguousarray(p.terms.reshape(-1, self.D)), np.ascontiguousarray(live.rows),
                                   dtype=self.dtype).reshape(6, -1, n)
            W = np.stack([XR.mix_scores(e[c], WEIGHTS[c]) for c in range(6)])
            best = lambda scores, s: np.sort(scores[s])[::-1]
            q_in = in_domain(q, self.dtype)
            t_in = in_domain(p.terms.reshape(-1, self.D), self.dtype).reshape(6, -1).all(axis=1)
            spans_sel = {name: SP.selection(spans, 6, lo, n) for name, spans in span_sets.items()}
            for i in range(6):
                for name, s in (("masked", sel), ("masked2", sel2), *spans_sel.items()):   # mask_ref.gap_ok at any k
                    must[name][i] = bool(q_in[i] and s[i].any() and SP.gap_ok(best(sc[i], s[i]), self.D, k))
                must["diverse"][i] = bool(q_in[i] and sel[i].any() and DR.flag0_ok(best(sc[i], sel[i]), POOL, self.D))
                for name, s in (("mix", np.ones(n, bool)), ("mix_masked", sel[i])):
                    must[name][i] = bool(t_in[i] and s.any() and XR.flag0_ok(best(W[i], s), k, self.D, XR.abs_sum(WEIGHTS[i])))
                Sb = BR.bias_scores_loop(sc[i], BIAS_W[i], BR.row_bias(cols, list(BIAS_INDEX), 6, lo, n, self.capacity)[i])
                for name, s in (("biased", np.ones(n, bool)), ("biased_masked", sel[i])):
                    must[name][i] = bool(q_in[i] and s.any() and BR.flag0_ok(best(Sb, s), k, self.D))
                for op, w, m in FOLD_CALLS:
                    wts = _fold_weights(WEIGHTS if w else None, p.terms)[i]
                    F, s = FR.fold_scores_loop(e[i], wts, op)[0], sel[i] if m else np.ones(n, bool)
                    must[fold_name(op, w, m)][i] = bool(t_in[i] and s.any() and FR.flag0_ok(best(F, s), k, self.D, FR.abs_max(wts)))
            s_in = in_domain(p.seqs.reshape(-1, self.D), self.dtype).reshape(6, -1).all(axis=1)
            for name, (sep, gap, m) in (*SEQ_CALLS.items(), ("seq_one", (1, None, False))):
                steps, ok = (q[:, None, :], q_in) if name == "seq_one" else (p.seqs, s_in)
                for i in range(6):          # seq_ref.margin above 4 eps_seq with the k exact peaks held
                    s = seq_sel[i:i + 1] if m else None
                    worst, held = SQ.margin(steps[i:i + 1], live.rows, k, SEQ_G, sep, self.dtype, tags=live.tags, sel=s,
                                            max_gap_ms=-1 if gap is None else gap)
                    must[name][i] = bool(ok[i] and (s is None or s.any()) and held and worst > 4)
        exp["must_certify"] = must
        return exp


def fold_name(op, weighted, masked):
    return f"fold_{op}{'_w' if weighted else ''}{'_masked' if masked else ''}"


def _fold_weights(weights, terms):
    return [[1.0] * terms.shape[1]] * terms.shape[0] if weights is None else weights


def boost_values(shown):
    """fp32 [len]: the values ``bias_of_rows`` is given for the rows ``shown`` (flat, -1 padded): 2.0 - 0.02 x the place
    where the row first occurs - distinct per row, descending, large enough to decide a ranking on their own; a row shown
    twice carries one value, so the order of the builder's stores does not matter."""
    shown = np.asarray(shown, np.int64).ravel()
    first = {}
    for i, r in enumerate(shown.tolist()):
        first.setdefault(r, i)
    return np.array([2.0 - 0.02 * first[r] for r in shown.tolist()], np.float32)


@functools.lru_cache(maxsize=8)
def _links(rows, ords, D, dtype, lo, k, first, count, min_gap, max_back):
    """span_ref.links_ref, a pure function of the window's bytes: 300 restricted rankings, computed once for the model and
    for whoever answers from an equal model (tests/test_lifecycle_cpu.py's fake)."""
    out = SP.links_ref(np.frombuffer(rows, np.uint16).reshape(-1, D), lo, k, first=first, count=count, min_gap=min_gap,
                       max_back=max_back, group_of=None if ords is None else np.frombuffer(ords, np.int64), dtype=dtype)
    for a in out:
        a.setflags(write=False)
    return out


def where(row, id, meta):
    """The ``mask_where`` predicate of the probes, over the id string and ``meta["i"]``: the provenance index parsed
    from the id (``s<batch>_p<index>``) is odd, and the metadata is that row's own."""
    return meta["i"] == id and int(id.rsplit("_p", 1)[1]) % 2 == 1


def in_domain(bits, dtype):
    """bool per row: the norm is 0 or lies in the certificate's domain."""
    nrm = np.linalg.norm(CL.from_bits(np.ascontiguousarray(bits), dtype).astype(np.float64), axis=-1)
    return (nrm == 0) | ((nrm >= DOMAIN[0]) & (nrm <= DOMAIN[1]))


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
          "group_scoped_uncertified_count", "clip_uncertified_count", "masked_uncertified_count", "span_uncertified_count",
          "mix_uncertified_count", "diverse_uncertified_count", "bias_uncertified_count", "fold_uncertified_count",
          "seq_uncertified_count")


def _pair(got_s, got_r, want, what):
    """One (scores, rows) answer against the oracle's (rows, scores)."""
    _same(got_r, want[0], what + " rows")
    assert _bits_equal(got_s, want[1]), what + " scores (bit-exact bar)"


def _certified(flags, must, what):
    """The flag-0 demand: the fast path may not leave to the redo a query that its own oracle condition says it must
    certify (the redo would hide a broken scan)."""
    flags = _np(flags)[:len(must)]
    bad = [i for i, m in enumerate(must) if m and flags[i] != 0]
    assert not bad, f"{what}: queries {bad} must be certified by the fast path, flags {flags.tolist()}"


def _masks(mem, io, p: Probes, exp, shown, carry, at):
    """The six masks of a checkpoint, built on ``mem``: -> the stacked masks ``[6, W]`` and the exclusion mask with its
    complement for the next checkpoint to carry.  ``rows_of_mask`` of every one must be the model's selection."""
    none = mem.new_mask()[0]
    excl = ~mem.mask_of_rows(shown)
    built = [~mem.new_mask()[0], mem.mask_of_scope(list(p.mask_scopes)), excl, mem.mask_where(where),
             *((none, none) if carry.get("masks") is None else carry["masks"])]
    names = ("all ones", "mask_of_scope", "~mask_of_rows", "mask_where", "carried ~mask_of_rows", "carried mask_of_rows")
    for name, m, want in zip(names, built, exp["mask_rows"]):
        got = np.asarray(mem.rows_of_mask(m), np.int64)
        assert np.array_equal(got, want), f"{at}rows_of_mask of the {name} mask: {got.tolist()} != {want.tolist()}"
    carry["built"] = (excl, ~excl)
    return io.stack(built)


def _bias(mem, io, model: Model, p: Probes, exp, shown, carry, at):
    """The four bias columns of a checkpoint as one stack ``[4, S]`` on ``mem``: zeros, ``bias_of_rows`` of the rows
    ``topk`` just returned (the device tensor, -1 padding and all), ``bias_of_age``, and the carried column.  The two the
    memory builds must be the model's arrays bit for bit at the slots of live rows (the other entries of ``bias_of_rows``
    are unspecified), and ``bias_of_age`` must leave its fill in every other slot."""
    lo, live = model.window()
    cols = mem.new_bias(4)
    mem.bias_of_rows(shown, [float(v) for v in boost_values(exp["topk"][0])], out=cols[1])
    mem.bias_of_age(p.bias_now, AGE_PER_MS, fill=AGE_FILL, out=cols[2])
    if carry.get("bias") is not None:
        cols[3][...] = carry["bias"]
    slots = (lo + np.arange(live.rows.shape[0], dtype=np.int64)) % model.capacity
    for i, name in ((1, "bias_of_rows"), (2, "bias_of_age")):
        got = np.ascontiguousarray(io.col_at(cols[i], slots), np.float32)
        assert np.array_equal(got.view(np.uint32), exp["bias_cols"][i][slots].view(np.uint32)), \
            f"{at}{name}: the column differs from the model's at the slots of live rows"
    dead = np.setdiff1d(np.arange(exp["bias_cols"].shape[1]), slots)
    assert (np.asarray(io.col_at(cols[2], dead)) == np.float32(AGE_FILL)).all(), at + "bias_of_age: a slot without a live row is not the fill"
    carry["built_bias"] = io.keep(cols[1])
    return cols


def _seq_answer(got, want, what):
    """(scores, rows, step_rows, step_scores) of the memory against the oracle's (rows, scores, step_rows, step_scores)."""
    s, r, sr, ss = got
    _pair(s, r, want, what)
    _same(sr, want[2], what + " step rows")
    assert _bits_equal(ss, want[3]), what + " step scores (bit-exact bar)"


def checkpoint(mem, model: Model, p: Probes, io, exp=None, label="", carry=None):
    """``mem`` against ``model``: the accessors, then the seventeen readers; -> the ``*_uncertified_count`` of every
    reader.  ``io`` carries what is not part of the memory's surface: ``t(bits)`` (bit patterns -> what the memory takes
    as rows), ``ordinals(mem)`` (the ordinal column of the live rows in row-id order, vm_memory_group_ordinals),
    ``raw(mem, n)`` (rows, tags, keys, ordinals over slots [0, n) in slot order), ``stack(masks)``, ``f64(x)`` and
    ``i64d(x)`` (what the memory takes as stacked masks, as a device fp64 and as a device int64 tensor), ``col_at(col,
    slots)`` (a bias column read back at the given slots) and ``keep(col)`` (a copy of a column that outlives its stack).
    ``carry``: a dict; ``carry["masks"]`` are the previous checkpoint's exclusion mask and its complement and
    ``carry["bias"]`` its ``bias_of_rows`` column as this memory built them (searched again now, stale), ``carry["built"]``
    and ``carry["built_bias"]`` receive this checkpoint's."""
    carry = {} if carry is None else carry
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

    # identities the model owes before any device answer counts: the all-ones mask, the (1, 0, 0) weights and lam = 1
    # change nothing
    assert MASK_INDEX[0] == 0 and WEIGHTS[0] == [1.0, 0.0, 0.0] and LAM[0] == 1.0
    for name in ("masked", "mix", "mix_masked"):
        assert np.array_equal(exp[name][0][0], exp["topk"][0][0]) and _bits_equal(exp[name][1][0], exp["topk"][1][0]), \
            f"{at}model: query 0 of {name} is not topk's"
    assert np.array_equal(exp["diverse"][0][0], exp["masked"][0][0]) and _bits_equal(exp["diverse"][1][0], exp["masked"][1][0]), \
        at + "model: lam = 1 is not topk_masked"
    # the zero column, a column index out of range and a weight of 0.0 are topk (with the masks: topk_masked); one step
    # with min_sep = 1 is topk
    assert BIAS_INDEX[0] == 0 and not 0 <= BIAS_INDEX[4] < 4 and BIAS_W[5] == 0.0 and BIAS_PLAIN == (0, 4, 5)
    for name, plain in (("biased", "topk"), ("biased_masked", "masked")):
        for i in BIAS_PLAIN:
            assert np.array_equal(exp[name][0][i], exp[plain][0][i]) and _bits_equal(exp[name][1][i], exp[plain][1][i]), \
                f"{at}model: query {i} of {name} is not {plain}'s"
    assert np.array_equal(exp["seq_one"][0], exp["topk"][0]) and _bits_equal(exp["seq_one"][1], exp["topk"][1]) and \
        np.array_equal(exp["seq_one"][2][:, :, 0], exp["topk"][0]), at + "model: J = 1, min_sep = 1 is not topk"
    must = exp["must_certify"]
    q, terms, lam, shown = io.t(p.queries), io.t(p.terms), io.f64(LAM), None
    for exact in (False, True):
        form = f"{at}{'exact' if exact else 'default'} "
        s, r = mem.topk(q, p.k, exact=exact)
        shown = shown if exact else r                   # the default form's rows, as returned: the exclusion mask's operand
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
        # ---- the readers whose operands speak about row ids and slots
        if not exact:
            masks = _masks(mem, io, p, exp, shown, carry, at)
        fast = (lambda flags, name: None) if exact else \
            (lambda flags, name: _certified(getattr(mem, flags), must[name], f"{form}{name} ({flags})"))
        for name, index in (("masked", MASK_INDEX), ("masked2", MASK_INDEX2)):
            s, r = mem.topk_masked(q, p.k, masks, mask_index=list(index), exact=exact)
            _pair(s, r, exp[name], form + f"topk_masked mask_index={list(index)}")
            fast("last_mask_flags", name)
        for name, spans in (("span", p.spans), ("span_carried", p.carried_span and [p.carried_span] * 6)):
            if spans is None:
                continue
            for given in (spans, io.i64d([[INT64_MIN if a is None else a, INT64_MAX if b is None else b] for a, b in spans])):
                s, r = mem.topk_span(q, p.k, given, exact=exact)
                _pair(s, r, exp[name], form + f"topk_span {name} {'host pairs' if given is spans else 'device tensor'}")
                fast("last_span_flags", name)
        for name, kw in (("mix", {}), ("mix_masked", {"mask": masks, "mask_index": list(MASK_INDEX)})):
            s, r = mem.topk_mix(terms, WEIGHTS, p.k, exact=exact, **kw)
            _pair(s, r, exp[name], form + f"topk_mix {name}")
            fast("last_mix_flags", name)
        s, r = mem.topk_diverse(q, p.k, pool=POOL, lam=lam, mask=masks, mask_index=list(MASK_INDEX), exact=exact)
        assert _bits_equal(mem.last_diverse_mmr, exp["diverse"][2]), form + "topk_diverse last_diverse_mmr"
        _pair(s, r, exp["diverse"], form + "topk_diverse")
        fast("last_diverse_flags", "diverse")
        for (back, own), want in zip(LINK_CALLS, exp["links"]):
            s, r = mem.recall_links(p.links[0], p.links[1], k=LINK_K, min_gap=LINK_GAP, max_back=back, exclude_group=own,
                                    block=LINK_BLOCK, exact=exact)
            _pair(s, r, want, form + f"recall_links max_back={back} exclude_group={own}")
        # ---- the biased, the any/all and the sequence search
        if not exact:
            bias = _bias(mem, io, model, p, exp, shown, carry, at)
            seq_masks = io.stack([*masks, ~mem.mask_of_rows([p.seq_excluded])])
            seqs, ones = io.t(p.seqs), io.t(p.queries[:, None, :])
        with_masks = {"mask": masks, "mask_index": list(MASK_INDEX)}
        for name, kw in (("biased", {}), ("biased_masked", with_masks)):
            s, r = mem.topk_biased(q, p.k, bias, weight=list(BIAS_W), bias_index=list(BIAS_INDEX), exact=exact, **kw)
            _pair(s, r, exp[name], form + f"topk_biased {name}")
            fast("last_bias_flags", name)
        for op, w, m in FOLD_CALLS:
            name = fold_name(op, w, m)
            s, r, t = mem.topk_fold(terms, p.k, op=op, weights=WEIGHTS if w else None, exact=exact, **(with_masks if m else {}))
            _pair(s, r, exp[name], form + f"topk_fold {name}")
            _same(t, exp[name][2], form + f"topk_fold {name} term indices")
            fast("last_fold_flags", name)
        for name, (sep, gap, m) in SEQ_CALLS.items():
            kw = {"mask": seq_masks, "mask_index": list(SEQ_MASK_INDEX)} if m else {}
            _seq_answer(mem.topk_seq(seqs, p.k, max_step=SEQ_G, min_sep=sep, max_gap_ms=gap, exact=exact, **kw), exp[name],
                        form + f"topk_seq {name}")
            fast("last_seq_flags", name)
        _seq_answer(mem.topk_seq(ones, p.k, max_step=SEQ_G, min_sep=1, exact=exact), exp["seq_one"], form + "topk_seq J=1")
        fast("last_seq_flags", "seq_one")
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
    planted scenes of ragged sizes 1 - 23 (tests/support.clustered, noise 0.3: rows of one scene score about
    0.92 against each other, rows of two scenes about 0).  f16: every row scaled by 2^u, u uniform in [-2, 2], so the
    row norms spread over a factor of 16 and a norm left on the wrong row shows (tests/test_erase_gpu._data); bf16:
    unit rows."""
    import torch
    from tests.support import clustered, group_sizes
    D = DIMS[dtype]
    sizes = group_sizes(330, "ragged", 11 if dtype == "f16" else 12)
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
        self.carry = {}                  # the last checkpoint's exclusion masks (the memory's, and the model's words), its
                                         # boost column (the memory's, and the model's array) and span: searched again,
                                         # stale, after the next mutation; a restored memory is a new object and starts
                                         # without them, a reset or an erase keeps them
        self.last_erase = None           # new_row_of of the erase since the last checkpoint

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
        self.last_erase = np.array(out.new_row_of)
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
        total = self.model.total
        spans = [(None, None), (None, lo + n // 2), (lo - 5, lo + 20), (total - 3, total + 10), (7, 3), (total - 1, total - 1)]
        # a mixed query: the probe query, the next one, and a row far from it - the row that is gone when there is one
        lost = self.overwritten if self.overwritten is not None else self.gone
        far = [np.array(self.src[lost]) if lost is not None else live.rows[int(np.argmin(sc[c]))] if n else spare[c]
               for c in range(6)]
        terms = np.stack([np.stack([q[c], q[(c + 1) % 6], far[c]]) for c in range(6)])
        w = min(n, LINK_ROWS)
        seqs, excluded = self.sequences(live, rnd)
        now = int(live.tags[-1]) & ((1 << MS_BITS) - 1) if n else 0
        return Probes(q, scopes, clips, range_min, mask_scopes=[one, window], carried=self.carry.get("words"), spans=spans,
                      carried_span=self.carry.get("span"), terms=terms, links=(total - w, w), bias_now=now,
                      carried_bias=self.carry.get("bias_col"), seqs=seqs, seq_excluded=excluded)

    def chains(self, live, rnd):
        """int64 [6, 4]: the live indices of the rows the six sequences are noisy copies of, from the model alone.
        (a) across the driver's ``join`` - rows j - 1 and j became adjacent in an erase - when there is one; (b) ends at
        the newest row; (c) begins at the oldest live row - in a wrapped ring whose slot 0 lies inside the window (every
        wrapped checkpoint but the one at exactly twice the capacity) around the row in slot 0 instead, so that its rows
        straddle slots capacity - 1 and 0; (d) around the first change of source, where no chain may hold them all; (e)
        four adjacent rows of one event, of which the sequence's mask leaves out the second; (f) around the probe query's
        row, searched under the carried mask."""
        n, m = live.rows.shape[0], self.model
        at = lambda first, gaps=(2, 1, 2): min(max(int(first), 0), n - 1 - sum(gaps)) + np.cumsum([0, *gaps])
        j = self.join if self.join is not None and 3 <= self.join <= n - 3 else n // 2
        w = (-m.base) % m.capacity                           # the live index of the row in slot 0
        cuts = np.nonzero((live.tags[1:] >> MS_BITS) != (live.tags[:-1] >> MS_BITS))[0] + 1
        starts = np.nonzero(np.concatenate([[True], live.keys[1:] != live.keys[:-1]]))[0]
        long = [int(s) for s, e in zip(starts, np.concatenate([starts[1:], [n]])) if e - s >= 6 and s >= n // 3]
        return np.stack([at(j - 3), at(n - 6), at(w - 3) if m.wrapped and 3 <= w <= n - 3 else at(0),
                         at(cuts[0] - 3) if cuts.size else at(n // 4), at((long[0] if long else n // 3) + 1, (1, 1, 1)),
                         at(rnd - 2)])

    def sequences(self, live, rnd):
        """-> (uint16 [6, 4, D] the sequences, the row id the mask of (e) leaves out or -1): seq_ref.steps_at of
        ``chains``; never-stored rows when fewer than 16 rows are live."""
        n = live.rows.shape[0]
        if n < 16:
            spare = self.bits[-6:]
            return np.stack([spare[[(i + j) % 6 for j in range(SEQ_J)]] for i in range(6)]), -1
        chains = self.chains(live, rnd)
        return SQ.steps_at(live.rows, self.dtype, chains, 7), self.model.base + int(chains[4, 1])

    def check(self, label):
        n = self.model.total - self.model.base
        assert n % 16 or n == 0, f"[{label}] {n} live rows: a multiple of 16 leaves no ragged tile"
        p = self.probes()
        exp = self.model.expect(p)
        for hook in self.hooks:
            hook(label, self, p, exp)
        carry = {"masks": self.carry.get("masks"), "bias": self.carry.get("bias")}
        self.log.append((label, checkpoint(self.mem, self.model, p, self.io, exp, label, carry)))
        shown = exp["topk"][0]
        words = MR.pack_rows(shown[shown >= 0], self.model.capacity)         # mask_of_rows of the rows shown, by the model
        self.carry = {"masks": carry["built"], "words": (~words, words),
                      "span": (self.model.base + 10, self.model.total - 10),
                      "bias": carry["built_bias"], "bias_col": exp["bias_cols"][1]}   # the memory's column, and the model's
        self.last_erase = None


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
