"""Sparse host model of a memory too large to rank on the host (tests/test_bigmem_gpu.py; DESIGN.md "Rows past 4 GiB").

A test helper, not a conftest.  The memory is NOISE rows with PLANTED rows written over some of them:

  noise    first half of the dims = 0.05 x a random unit vector, second half = a random unit vector.  A query whose second
           half is zero then has |cosine| <= ||first half|| / ||row|| <= NOISE_BOUND against it (Cauchy-Schwarz), whatever
           the values are; ``noise_ratio`` measures that quotient on the rounded rows and the builder asserts it per block.
  planted  supported on the first half: member (f, j) of family f is  c q_f + sqrt(1 - c^2) u,  c = 0.95 - 0.05 j,  with
           the 16 base queries q_f orthonormal and u orthogonal to all of them: it scores c against q_f and 0 against
           every other base query.  ``positions`` puts the members around the boundaries b1 and b2 (2 GiB and 4 GiB in
           the large layout), at a control site far below b1, at rows 0 - 1 and at the tail.

The model keeps only the NEIGHBOURHOODS of those sites (planted and noise rows alike, as bits) with their row ids, keys
and tags.  Every expectation is the search's own oracle (oracle.cref, tests/*_ref.py) over the neighbourhood rows, its
indices mapped to row ids; the map is monotone, so (score desc, row asc) survives it.  That equals the oracle over ALL rows
exactly when no other row can enter the answer, which ``Sparse`` asserts from the oracle's own numbers: every returned
score is at least FLOOR, and every row left out is noise, bounded by NOISE_BOUND x the query's weight.  Construction
parameters, asserted on every run, never tuned.  tests/test_bigmem_cpu.py proves the reasoning on a layout small enough for
the dense oracle.

The biased search adds what a bias column may hold on the rows left out (``Column``: known at the candidates' slots, bounded
everywhere else), the sequence search how far a chain reaches into a run (``Sparse.seq``).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from oracle import cref
from tests import bias_ref as BR
from tests import clip_ref as CL
from tests import diverse_ref as DR
from tests import fold_ref as FR
from tests import group_ref as G
from tests import group_scope_ref as GS
from tests import mask_ref as MR
from tests import mix_ref as XR
from tests import range_ref as R
from tests import scope_ref as S
from tests import seq_ref as SQ
from tests import span_ref as SP
from tests import summary_ref as M
from tests import events_ref as V
from tests.scored_ref import slack_m
from tests.support import to_bits

NOISE_SCALE, NOISE_BOUND, FLOOR, SPACING = 0.05, 0.06, 0.5, 0.05
FAMILIES, LEVELS, GROUP, MS_BITS = 16, 9, 8, 40
HOOD = 48                      # a neighbourhood reaches this far to either side of its site
DTYPE = "f16"


class Layout(NamedTuple):
    N: int                     # live rows
    D: int
    b1: int                    # the first boundary row (byte offset 2^31 in BIG)
    b2: int                    # the second (byte offset 2^32, element offset 2^31)
    ctrl: int                  # the control site, far below b1
    source_rows: int           # rows per source: the tag of row r is make_tag(r // source_rows, r)
    block: int                 # rows generated and appended at a time
    spare: int                 # capacity - N


BIG = Layout((1 << 21) + 70_003, 1024, 1 << 20, 1 << 21, 300_000, 262_144, 65_536, 4096)
SMALL = Layout(6000, 128, 2048, 4096, 600, 512, 1000, 64)


def tag_of(L: Layout, rows):
    rows = np.asarray(rows, np.int64)
    return ((rows // L.source_rows) << MS_BITS) | rows


def scope_of_source(first, last=None):
    """The inclusive tag range of sources first .. last."""
    last = first if last is None else last
    return (int(first) << MS_BITS, (int(last) << MS_BITS) | ((1 << MS_BITS) - 1))


def positions(L: Layout) -> dict:
    """row id -> (family, level).  Level j scores 0.95 - 0.05 j; level -1 (rows 0 and 1) is the base query itself.
    Levels 0 and 6 of a family share one 8-row group just above b2 (the grouped search must return only the better);
    every family has members on both sides of b1 and of b2, at the control site and at the tail."""
    out = {0: (0, -1), 1: (1, -1)}
    for f in range(FAMILIES):
        out[L.b2 + 2 * f] = (f, 0)
        out[L.b1 - 16 + f] = (f, 1)
        out[L.N - 16 + f] = (f, 2)
        out[L.ctrl - 16 + f] = (f, 3)
        out[L.b2 - 16 + f] = (f, 4)
        out[L.b1 + f] = (f, 5)
        out[L.b2 + 2 * f + 1] = (f, 6)
        out[L.ctrl + f] = (f, 7)
        out[L.b1 + 16 + f] = (f, 8)
    assert len(out) == 2 + FAMILIES * LEVELS
    return out


def members(L: Layout, f: int) -> dict:
    """level -> row id of family f."""
    return {j: r for r, (ff, j) in positions(L).items() if ff == f}


def hoods(L: Layout):
    """The neighbourhoods [lo, hi), ascending and disjoint, cut at group boundaries."""
    cut = lambda a, b: (max(0, a) // GROUP * GROUP, min(L.N, b))
    out = [cut(0, 2 * HOOD), cut(L.ctrl - HOOD, L.ctrl + HOOD), cut(L.b1 - HOOD, L.b1 + HOOD),
           cut(L.b2 - HOOD, L.b2 + HOOD), cut(L.N - 2 * HOOD, L.N)]
    assert all(a[1] < b[0] for a, b in zip(out, out[1:]))
    pos = positions(L)
    for r in pos:   # a planted row lies at least 8 rows inside its neighbourhood (a clip window that leaves one is noise)
        assert any(lo + (8 if lo else 0) <= r < hi - (8 if hi < L.N else 0) for lo, hi in out), r
    return out


def from_bits(b, dtype=DTYPE) -> np.ndarray:
    if dtype == "f16":
        return np.ascontiguousarray(b).view(np.float16).astype(np.float64)
    return CL.from_bits(np.ascontiguousarray(b), dtype).astype(np.float64)


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def base_queries(L: Layout, seed=5) -> np.ndarray:
    """fp64 [16, D / 2]: orthonormal."""
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((L.D // 2, FAMILIES)))
    return q.T.copy()


def planted_rows(L: Layout, seed=5, dtype=DTYPE) -> dict:
    """row id -> bits [D]."""
    h = L.D // 2
    B = base_queries(L, seed)
    rng = np.random.default_rng(seed + 1)
    out = {}
    for r, (f, j) in sorted(positions(L).items()):
        u = rng.standard_normal(h)
        u = _unit(u - B.T @ (B @ u))
        c = 1.0 if j < 0 else 0.95 - SPACING * j
        v = np.zeros(L.D)
        v[:h] = c * B[f] + np.sqrt(1.0 - c * c) * u
        out[r] = to_bits(v, dtype)
    return out


def queries(L: Layout, Q: int, seed: int, noise=0.02, dtype=DTYPE) -> np.ndarray:
    """bits [Q, D]: query i is base query i % 16 plus a small fresh perturbation, first half only."""
    h = L.D // 2
    B = base_queries(L)
    rng = np.random.default_rng(1000 + seed)
    v = np.zeros((Q, L.D))
    v[:, :h] = B[np.arange(Q) % FAMILIES] + noise * _unit(rng.standard_normal((Q, h)))
    return to_bits(v, dtype)


def noisy_copy(bits, seed, noise=0.05) -> np.ndarray:
    """Planted rows again with a small perturbation of the first half (clip frames, near-duplicates)."""
    x = from_bits(bits)
    h = x.shape[-1] // 2
    assert not x[..., h:].any()
    e = np.zeros_like(x)
    e[..., :h] = noise * _unit(np.random.default_rng(2000 + seed).standard_normal(x[..., :h].shape))
    return to_bits(x + e, DTYPE)


def first_half_only(bits) -> bool:
    """What every query, clip frame and mix term must be for NOISE_BOUND to hold (a zero has the bits 0x0000 or 0x8000 in
    both 16-bit types)."""
    return not (np.asarray(bits)[..., bits.shape[-1] // 2:] & 0x7FFF).any()


# ---- the rows ------------------------------------------------------------------------------------------------------------
def noise_block(n, D, gen, device, dtype=DTYPE):
    """16-bit tensor [n, D] on ``device`` from the seeded generator ``gen`` of that device."""
    import torch
    h = D // 2
    a = torch.randn((n, h), generator=gen, device=device)
    b = torch.randn((n, h), generator=gen, device=device)
    a, b = a / a.norm(dim=1, keepdim=True), b / b.norm(dim=1, keepdim=True)
    return torch.cat([NOISE_SCALE * a, b], dim=1).to(torch.float16 if dtype == "f16" else torch.bfloat16)


def noise_ratio(x16):
    """||first half|| / ||row|| of fp16 rows, in fp32 on their device: the bound on |cosine| against a first-half query."""
    f = x16.float()
    return f[:, :f.shape[1] // 2].norm(dim=1) / f.norm(dim=1)


def blocks(L: Layout, gen, device, first=0, total=None, dtype=DTYPE):
    """Yields (start, rows fp16 [n, D], keys int64 [n], tags int64 [n]) on ``device`` for rows first .. total - 1: fresh
    noise per block, the planted rows written over it, the noise bound asserted on what is left."""
    import torch
    plant = planted_rows(L, dtype=dtype)
    total = L.N if total is None else total
    for start in range(first, total, L.block):
        n = min(L.block, total - start)
        x = noise_block(n, L.D, gen, device, dtype)
        worst = float(noise_ratio(x).max())
        assert worst <= NOISE_BOUND, f"block at {start}: noise ratio {worst}"
        here = [r for r in plant if start <= r < start + n]
        if here:
            b = np.stack([plant[r] for r in here]).view(np.int16)
            x[torch.tensor([r - start for r in here], device=device)] = torch.from_numpy(b).view(x.dtype).to(device)
        ids = torch.arange(start, start + n, dtype=torch.int64, device=device)
        yield start, x, ids // GROUP, ((ids // L.source_rows) << MS_BITS) | ids


def cut_hoods(L: Layout, start, x, into: dict):
    """Copies the bits of every neighbourhood row of the block into ``into`` (row id -> bits)."""
    import torch
    n = x.shape[0]
    for lo, hi in hoods(L):
        a, b = max(lo, start), min(hi, start + n)
        if a < b:
            part = x[a - start:b - start].contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
            for i, r in enumerate(range(a, b)):
                into[r] = part[i].copy()


# ---- the model -----------------------------------------------------------------------------------------------------------
class Sparse:
    """The candidate rows of a memory of ``total`` live rows: ``gid`` their row ids (ascending), ``rows`` their bits,
    ``keys`` and ``tags``; ``planted`` bool: which of them are planted (the others must satisfy the noise bound);
    ``newest_ms`` the largest clock of any row, candidate or not."""

    def __init__(self, L: Layout, cand: dict, total=None, base=0, dtype=DTYPE):
        self.L, self.D, self.dtype = L, L.D, dtype
        self.gid = np.array(sorted(cand), np.int64)
        self.rows = np.stack([cand[int(r)] for r in self.gid])
        self.keys = self.gid // GROUP
        self.tags = tag_of(L, self.gid)
        pos = positions(L)
        self.planted = np.array([int(r) in pos for r in self.gid])
        self.total = L.N if total is None else total
        self.base = base
        self.newest_ms = self.total - 1       # tag_of: the clock of a row of the recipe is the row id it is appended with
        self.check_noise()

    def check_noise(self):
        x = from_bits(self.rows[~self.planted], self.dtype)
        ratio = np.linalg.norm(x[:, :self.D // 2], axis=1) / np.linalg.norm(x, axis=1)
        assert (ratio <= NOISE_BOUND).all(), float(ratio.max())

    # ---- state changes
    def erase(self, ids):
        """vm_memory_erase_rows of candidate rows -> new_row_of at every OLD candidate id (dict)."""
        ids = sorted(set(int(r) for r in ids))
        assert all(r in set(self.gid.tolist()) for r in ids), "the model only knows how to erase candidate rows"
        old = self.gid.copy()
        shift = np.searchsorted(np.array(ids), old, side="left")        # erased rows below each candidate
        new = np.where(np.isin(old, ids), -1, old - shift)
        keep = new >= 0
        for name in ("rows", "keys", "tags", "planted"):
            setattr(self, name, getattr(self, name)[keep])
        self.gid = new[keep]
        self.total -= len(ids)
        return dict(zip(old.tolist(), new.tolist()))

    def append(self, bits, keys, tags):
        n = bits.shape[0]
        self.gid = np.concatenate([self.gid, self.total + np.arange(n)])
        self.rows = np.concatenate([self.rows, bits])
        self.keys = np.concatenate([self.keys, np.asarray(keys, np.int64)])
        self.tags = np.concatenate([self.tags, np.asarray(tags, np.int64)])
        self.planted = np.concatenate([self.planted, np.ones(n, bool)])
        self.total += n
        self.newest_ms = max(self.newest_ms, int((np.asarray(tags, np.int64) & BR.TAG_MS_MASK).max()))

    def drop_below(self, base):
        """A ring overwrote every row below ``base``."""
        keep = self.gid >= base
        for name in ("rows", "keys", "tags", "planted", "gid"):
            setattr(self, name, getattr(self, name)[keep])
        self.base = base

    # ---- helpers
    def at(self, row):
        i = int(np.searchsorted(self.gid, row))
        assert self.gid[i] == row, row
        return i

    def _ids(self, r):
        r = np.asarray(r, np.int64)
        return np.where(r >= 0, self.gid[np.maximum(r, 0)], -1)

    def segments(self):
        """[a, b) index runs of consecutive row ids."""
        cuts = np.nonzero(np.diff(self.gid) != 1)[0] + 1
        return list(zip(np.concatenate([[0], cuts]).tolist(), np.concatenate([cuts, [self.gid.size]]).tolist()))

    def scores(self, q):
        return cref.cosine_matrix(np.ascontiguousarray(q), np.ascontiguousarray(self.rows), dtype=self.dtype)

    def _safe(self, q, r, s, what, weight=1.0, full=True):
        """No row outside the candidates can enter: the operands are first-half only, every returned score is at least
        FLOOR (``full``: and none is missing), and FLOOR is above the most a noise row can score."""
        assert first_half_only(q), what + ": an operand has a nonzero second half"
        assert NOISE_BOUND * weight < FLOOR, what
        r, s = np.asarray(r), np.asarray(s)
        if full:
            assert (r >= 0).all(), what + ": the candidates do not fill the answer"
        assert (s[r >= 0] >= FLOOR).all(), f"{what}: worst expected score {s[r >= 0].min()} below {FLOOR}"

    def _gaps(self, q, sel, k, what):
        sc = self.scores(q)
        for i in range(sc.shape[0]):
            best = np.sort(sc[i][sel[i]])[::-1]
            assert SP.gap_ok(best, self.D, k), f"{what}: query {i} may be left to the redo"

    def _group_gaps(self, q, sel, k, what):
        """``_gaps`` for the grouped searches: on each group's best selected score (every group of the candidates is
        whole: ``hoods`` cuts at group boundaries)."""
        sc, grp = self.scores(q), G.group_ids(self.keys)
        for i in range(sc.shape[0]):
            best = np.sort([sc[i][(grp == g) & sel[i]].max() for g in np.unique(grp[sel[i]])])[::-1]
            assert SP.gap_ok(best, self.D, k), f"{what}: query {i} may be left to the redo"

    def _all(self, Q):
        return np.ones((Q, self.gid.size), bool)

    # ---- expectations: each search's own oracle on the candidates
    def topk(self, q, k, min_score=None):
        """``min_score``: above the noise bound; the answer may then be short (k beyond a family's members)."""
        assert min_score is None or min_score > NOISE_BOUND
        r, s = cref.cosine_topk(np.ascontiguousarray(q), np.ascontiguousarray(self.rows), k, dtype=self.dtype,
                                min_score=min_score)
        self._safe(q, r, s, "topk", full=min_score is None)
        if min_score is None:
            self._gaps(q, self._all(q.shape[0]), k, "topk")
        return self._ids(r), s

    def scoped(self, q, scopes, k):
        r, s = S.scoped_topk(q, self.rows, self.tags, scopes, k, dtype=self.dtype)
        self._safe(q, r, s, "scoped")
        lo, hi = S.scope_arrays(scopes, q.shape[0])
        self._gaps(q, np.stack([S.scope_mask(self.tags, lo[i], hi[i]) for i in range(q.shape[0])]), k, "scoped")
        return self._ids(r), s

    def grouped(self, q, k):
        r, s, kk = G.grouped_topk(q, np.ascontiguousarray(self.rows), self.keys, k, dtype=self.dtype)
        self._safe(q, r, s, "grouped")
        self._group_gaps(q, self._all(q.shape[0]), k, "grouped")
        return self._ids(r), s, kk

    def grouped_scoped(self, q, scopes, k):
        r, s, kk = GS.group_scoped_topk(q, np.ascontiguousarray(self.rows), self.keys, self.tags, scopes, k, dtype=self.dtype)
        self._safe(q, r, s, "grouped_scoped")
        lo, hi = S.scope_arrays(scopes, q.shape[0])
        self._group_gaps(q, np.stack([S.scope_mask(self.tags, lo[i], hi[i]) for i in range(q.shape[0])]), k, "grouped_scoped")
        return self._ids(r), s, kk

    def sel_of_rows(self, ids, Q):
        return np.tile(np.isin(self.gid, np.asarray(ids, np.int64)), (Q, 1))

    def sel_of_scope(self, scope, Q):
        return np.tile(S.scope_mask(self.tags, *scope), (Q, 1))

    def masked(self, q, sel, k):
        r, s = MR.masked_topk(q, self.rows, sel, k, dtype=self.dtype)
        self._safe(q, r, s, "masked")
        self._gaps(q, sel, k, "masked")
        return self._ids(r), s

    def local_spans(self, spans, Q):
        """Row-id spans -> inclusive index spans among the candidates (the map is monotone)."""
        return [(int(np.searchsorted(self.gid, max(lo, -1), "left")), int(np.searchsorted(self.gid, hi, "right")) - 1)
                for lo, hi in SP.pairs(spans, Q)]

    def span(self, q, spans, k):
        loc = self.local_spans(spans, q.shape[0])
        r, s = SP.span_topk(q, self.rows, loc, k, dtype=self.dtype)
        self._safe(q, r, s, "span")
        self._gaps(q, SP.selection(loc, q.shape[0], 0, self.gid.size), k, "span")
        return self._ids(r), s

    def range(self, q, min_score, scopes=None):
        assert NOISE_BOUND < min_score < FLOOR
        hits = R.range_hits(q, self.rows, min_score, self.tags, scopes, dtype=self.dtype)
        out = []
        for r, s, c in hits:        # every hit is at or above the floor: a planted member, never a row near the threshold
            self._safe(q, r, s, "range", full=False)
            out.append((self.gid[r], s, c))
        return out

    def clip(self, clips, k, min_sep, min_score=None, scopes=None, max_gap_ms=-1):
        """-> (rows [C,k], scores [C,k], must bool [C]).  clip_ref.clip_topk per run of consecutive candidates, merged by
        (score desc, row asc).  A window that is not inside one run holds only noise frames (``hoods``: planted rows lie 8
        rows inside, L <= 8), so its W is at most NOISE_BOUND: below ``min_score`` when there is one, below every
        expected W otherwise (asserted).

        ``must``: clip_ref.margin's condition over the merged candidates with the windows left out bounded by
        NOISE_BOUND - among the best M possible peaks are k exact peaks, and the k-th clears max(the (M+1)-th best
        possible candidate window, NOISE_BOUND) by more than 2 eps_w.  The fast path must then certify the clip."""
        C, Lc = clips.shape[0], clips.shape[1]
        assert first_half_only(clips) and Lc <= 8 and (min_score is None or NOISE_BOUND < min_score)
        segs = [(a, b) for a, b in self.segments() if b - a >= Lc]
        for a, b in self.segments():      # unless the run ends where the memory does, its outermost L - 1 rows are noise
            if self.gid[a] != self.base:
                assert not self.planted[a:min(a + Lc - 1, b)].any(), f"a planted row just above {self.gid[a]}"
            if self.gid[b - 1] != self.total - 1:
                assert not self.planted[max(b - Lc + 1, a):b].any(), f"a planted row just below {self.gid[b - 1]}"
        out_r = np.full((C, k), -1, np.int64)
        out_s = np.zeros((C, k), np.float64)
        must = np.zeros(C, bool)
        parts = [CL.clip_topk(clips, self.rows[a:b], k, min_sep, dtype=self.dtype, tags=self.tags[a:b], scopes=scopes,
                              max_gap_ms=max_gap_ms, min_score=min_score, base=0) + (a,) for a, b in segs]
        lo, hi = CL.scope_arrays(scopes, C)
        Mk, e = k + max(k // 4, 8), CL.eps_w(self.D)
        for c in range(C):
            r = np.concatenate([np.where(p[0][c] >= 0, self.gid[np.maximum(p[0][c], 0) + p[2]], -1) for p in parts])
            s = np.concatenate([p[1][c] for p in parts])
            r, s = r[r >= 0], s[r >= 0]
            order = np.lexsort((r, -s))[:k]
            out_r[c, :order.size], out_s[c, :order.size] = r[order], s[order]
            if min_score is None:
                assert order.size == k and (s[order] > NOISE_BOUND).all(), "clip: a noise window could enter the answer"
            else:
                assert (s[order] > min_score).all()      # the filter, in the oracle: above anything a noise window reaches
            Ws, poss, peaks = [], [], []
            for a, b in segs:                            # clip_ref.margin's sets, run by run
                W = CL.window_scores(CL.frame_scores(clips[c], self.rows[a:b], self.dtype), Lc)
                ok = CL.window_mask(b - a, Lc, self.tags[a:b], None if lo is None else lo[c], None if hi is None else hi[c],
                                    max_gap_ms)
                far = np.zeros(W.size, bool)
                for d in range(1, min(min_sep, W.size)):
                    far[d:] |= ok[:-d] & (W[:-d] > W[d:] + 4 * e)
                    far[:-d] |= ok[d:] & (W[d:] > W[:-d] + 4 * e)
                Ws.append(W), poss.append(ok & ~far), peaks.append(CL.peak_mask(W, ok, min_sep))
            W, pos, pk = np.concatenate(Ws), np.concatenate(poss), np.concatenate(peaks)
            ids = np.nonzero(pos)[0]                     # run order = row order
            ranked = ids[np.lexsort((ids, -W[ids]))]
            exact = ranked[:Mk][pk[ranked[:Mk]]]
            if exact.size >= k:
                rest = max(W[ranked[Mk]] if ranked.size > Mk else -np.inf, NOISE_BOUND)
                must[c] = (W[exact[k - 1]] - rest) / e > 2
        return out_r, out_s, must

    # ---- the two whole-memory passes
    def summaries(self) -> "M.Summary":
        """summary_ref.summarize of every run of candidates (runs begin and end at group boundaries)."""
        parts = [M.summarize(self.rows[a:b], self.keys[a:b], self.dtype, base=int(self.gid[a])) for a, b in self.segments()]
        return M.Summary(*[np.concatenate([getattr(p, name) for p in parts]) for name in M.Summary._fields])

    def inner(self):
        """[lo, hi) row-id ranges of the rows whose link to the row before lies inside one run of candidates."""
        return [(int(self.gid[a]) + 1, int(self.gid[b - 1]) + 1) for a, b in self.segments()]

    def events(self, threshold, bound):
        """-> (event count, event_of at every candidate, the first row of that event).  PRECONDITION, which the caller
        shows over all rows: every link that is not inside one run (``inner``) is below ``bound`` <= threshold, so each
        such row opens an event.  Inside a run the links and the rule are events_ref's; no link lies within 0.02 above the
        threshold or between the bound and it."""
        assert bound <= threshold
        closed = []                                       # rows that continue the event of the row before
        for a, b in self.segments():
            link = V.links(self.rows[a:b], self.dtype)
            assert ((link[1:] > threshold + 0.02) | (link[1:] < bound)).all(), "a link near the threshold"
            o = V.opens(link, threshold, self.tags[a:b], -1)
            closed += [int(self.gid[a + i]) for i in range(1, b - a) if not o[i]]
        closed = np.array(sorted(closed), np.int64)
        n = self.total - self.base
        event_of = (self.gid - self.base) - np.searchsorted(closed, self.gid, "right")
        first = self.gid.copy()
        while np.isin(first, closed).any():
            first = np.where(np.isin(first, closed), first - 1, first)
        return n - closed.size, event_of, first, closed

    def mix(self, terms, weights, k, sel=None):
        C, J = terms.shape[0], terms.shape[1]
        r, s = XR.mix_topk(terms, weights, self.rows, sel, k, dtype=self.dtype)
        A = max(XR.abs_sum(w) for w in weights)
        self._safe(terms, r, s, "mix", weight=A)
        e = cref.cosine_matrix(terms.reshape(C * J, self.D), np.ascontiguousarray(self.rows), dtype=self.dtype).reshape(C, J, -1)
        for c in range(C):
            W = XR.mix_scores(e[c], weights[c])
            best = np.sort(W if sel is None else W[sel[c]])[::-1]
            assert XR.flag0_ok(best, k, self.D, XR.abs_sum(weights[c])), f"mix: query {c} may be left to the redo"
        return self._ids(r), s

    def diverse(self, q, k, pool, lam, sel=None):
        r, s, v = DR.diverse_topk(q, self.rows, sel, k, pool, list(lam), dtype=self.dtype)
        pr, ps = MR.masked_topk(q, self.rows, self._all(q.shape[0]) if sel is None else sel, pool, dtype=self.dtype)
        self._safe(q, pr, ps, "diverse pool")
        sc = self.scores(q)
        for i in range(q.shape[0]):
            best = np.sort(sc[i] if sel is None else sc[i][sel[i]])[::-1]
            assert DR.flag0_ok(best, pool, self.D), f"diverse: query {i} may be left to the redo"
        return self._ids(r), s, v

    # ---- the biased search: a column is known at the candidates' slots and bounded everywhere else
    def col_of_rows(self, ids, values, capacity) -> "Column":
        """``bias_of_rows(ids, values)``: bias_ref.bias_from_rows_ref, read at the candidates' slots.  Every id must be a
        candidate, so every other live slot holds 0."""
        live = [int(r) for r in ids if self.base <= int(r) < self.total]
        assert np.isin(live, self.gid).all(), "the model only knows a boost of candidate rows"
        col = BR.bias_from_rows_ref(ids, values, self.base, self.total - self.base, capacity)
        return Column(col[self.gid % capacity], 0.0, 0.0)

    def col_of_age(self, now_ms, per_ms, fill, capacity) -> "Column":
        """``bias_of_age(now_ms, per_ms, fill)``: bias_ref.bias_from_tags_ref per run, read at the candidates' slots.
        Everywhere else, in closed form: a row that is not a candidate was appended by the layout's recipe, so its clock
        is the row id it was appended with, in [0, newest]; with per_ms > 0 and now_ms >= newest its entry
        fl32(per_ms (clock - now_ms)) lies in [fl32(-per_ms now_ms), 0] (rounding is monotone)."""
        assert per_ms > 0 and now_ms >= self.newest_ms >= int((self.tags & BR.TAG_MS_MASK).max())
        at = np.zeros(self.gid.size, np.float32)
        for a, b in self.segments():
            col = BR.bias_from_tags_ref(self.tags[a:b], int(self.gid[a]), capacity, now_ms, per_ms, fill)
            at[a:b] = col[self.gid[a:b] % capacity]
        assert (at <= 0).all()
        return Column(at, float(np.float32(float(per_ms) * float(-int(now_ms)))), 0.0)

    def biased(self, q, cols, bias_index, betas, k, sel=None):
        """bias_ref.bias_topk_from_cosines on the candidates.  A row that is not a candidate scores at most
        NOISE_BOUND + max(beta lo, beta hi) of its query's column (an index out of range is the zero column): that must
        lie below the worst returned S.  The fast path must then certify every query whose ranks k and M + 1 stand
        bias_ref.flag0_ok apart, the rows left out taken at that bound (asserted: ``_flags0`` holds for all)."""
        Q, n = q.shape[0], self.gid.size
        assert first_half_only(q), "biased: an operand has a nonzero second half"
        e = self.scores(q)
        b, out = np.zeros((Q, n), np.float32), np.zeros(Q)
        for i, c in enumerate(bias_index):
            if 0 <= int(c) < len(cols):
                b[i] = cols[int(c)].at
                out[i] = max(float(betas[i]) * cols[int(c)].lo, float(betas[i]) * cols[int(c)].hi)
        r, s = BR.bias_topk_from_cosines(e, list(betas), b, sel, k)
        assert (r >= 0).all(), "biased: the candidates do not fill the answer"
        for i in range(Q):
            bound = NOISE_BOUND + out[i]
            assert bound < s[i].min(), f"biased: a row outside the candidates may score {bound}, query {i} returns {s[i].min()}"
            S = BR.bias_scores_loop(e[i], betas[i], b[i])
            best = np.sort(np.concatenate([S if sel is None else S[sel[i]], np.full(slack_m(k) + 1, bound)]))[::-1]
            assert BR.flag0_ok(best, k, self.D), f"biased: query {i} may be left to the redo"
        return self._ids(r), s

    # ---- the any/all search
    def fold(self, terms, weights, k, op, sel=None):
        """``mix``'s proof for fold_ref.fold_topk: |w_j e_j| <= A x NOISE_BOUND on a noise row for every term, so its
        max and its min are; every returned F is at least FLOOR.  For ``min`` that needs every term of a query to be a
        family with a member in the answer's rows: a term of another family scores about 0 there and the floor says so."""
        C, J = terms.shape[0], terms.shape[1]
        r, s, t = FR.fold_topk(terms, weights, self.rows, sel, k, op, dtype=self.dtype)
        self._safe(terms, r, s, "fold " + op, weight=max(FR.abs_max(w) for w in weights))
        e = cref.cosine_matrix(terms.reshape(C * J, self.D), np.ascontiguousarray(self.rows), dtype=self.dtype).reshape(C, J, -1)
        for c in range(C):
            A = FR.abs_max(weights[c])
            F, _ = FR.fold_scores_loop(e[c], weights[c], op)
            best = np.sort(np.concatenate([F if sel is None else F[sel[c]], np.full(slack_m(k) + 1, A * NOISE_BOUND)]))[::-1]
            assert FR.flag0_ok(best, k, self.D, A), f"fold {op}: query {c} may be left to the redo"
        return self._ids(r), s, t

    # ---- the sequence search
    def seq(self, steps, k, G, min_sep, sel=None, min_score=None, max_gap_ms=-1):
        """-> (end rows [C,k], scores [C,k], step rows [C,k,J], step scores [C,k,J], must bool [C]).  seq_ref.seq_topk per
        run of consecutive candidates, merged by (score desc, end row asc).

        Sound when every planted row a sequence may use (``sel`` [C, candidates]: its mask; rows that are no candidates
        count as selected) lies at least (J-1) G rows inside its run on both sides, unless the run ends where the memory
        does (asserted).  A chain reaches back (J-1) G rows at the most, so a chain that ends outside a run, or in a run's
        first (J-1) G rows, holds noise rows only and its A is at most NOISE_BOUND; inside, a run computes an end row's A
        from the whole chain or, in those first rows, from fewer chains of noise rows: at most NOISE_BOUND either way.
        Such an end row neither enters an answer whose scores are all above NOISE_BOUND (asserted; above ``min_score``
        when there is one) nor suppresses one.

        ``must``: seq_ref.margin's condition over the merged runs with the end rows left out bounded by NOISE_BOUND - among
        the best M possible peaks are k exact peaks, and the k-th clears max(the (M+1)-th best possible end row,
        NOISE_BOUND) by more than 4 eps_seq (the rule of tests/test_seq_gpu.py).  The fast path must then certify."""
        C, J = steps.shape[0], steps.shape[1]
        n, reach = self.gid.size, (J - 1) * G
        assert first_half_only(steps) and (min_score is None or NOISE_BOUND < min_score)
        el = SQ.eligible(n, C, sel)
        segs = self.segments()
        for a, b in segs:
            for c in range(C):
                p = self.planted[a:b] & el[c, a:b]
                if self.gid[a] != self.base:
                    assert not p[:reach].any(), f"sequence {c}: a planted row within {reach} rows above {self.gid[a]}"
                if self.gid[b - 1] != self.total - 1:
                    assert not p[max(b - a - reach, 0):].any(), f"sequence {c}: a planted row within {reach} rows below {self.gid[b - 1]}"
        parts = [SQ.seq_topk(steps, self.rows[a:b], k, G, min_sep, dtype=self.dtype, tags=self.tags[a:b], sel=el[:, a:b],
                             max_gap_ms=max_gap_ms, min_score=min_score, base=0) + (a,) for a, b in segs]
        out_r, out_s = np.full((C, k), -1, np.int64), np.zeros((C, k), np.float64)
        out_sr, out_ss = np.full((C, k, J), -1, np.int64), np.zeros((C, k, J), np.float64)
        must = np.zeros(C, bool)
        M, e = slack_m(k), SQ.eps_seq(self.D, J)
        for c in range(C):
            hit = [p[0][c] >= 0 for p in parts]
            r = np.concatenate([self.gid[p[0][c][h] + p[4]] for p, h in zip(parts, hit)])
            s = np.concatenate([p[1][c][h] for p, h in zip(parts, hit)])
            sr = np.concatenate([self.gid[p[2][c][h] + p[4]] for p, h in zip(parts, hit)])
            ss = np.concatenate([p[3][c][h] for p, h in zip(parts, hit)])
            order = np.lexsort((r, -s))[:k]
            m = order.size
            out_r[c, :m], out_s[c, :m], out_sr[c, :m], out_ss[c, :m] = r[order], s[order], sr[order], ss[order]
            if min_score is None:
                assert m == k and (s[order] > NOISE_BOUND).all(), "seq: an end row of noise chains could enter the answer"
            else:
                assert (s[order] > min_score).all()
            As, poss, peaks = [], [], []
            for a, b in segs:                            # seq_ref.margin's sets, run by run
                A, ok, _ = SQ.end_scores(CL.frame_scores(steps[c], self.rows[a:b], self.dtype), el[c, a:b],
                                         CL.tag_breaks(self.tags[a:b], max_gap_ms), G)
                far = np.zeros(b - a, bool)
                with np.errstate(invalid="ignore"):
                    for d in range(1, min(min_sep, b - a)):
                        far[d:] |= ok[:-d] & (A[:-d] > A[d:] + 4 * e)
                        far[:-d] |= ok[d:] & (A[d:] > A[:-d] + 4 * e)
                As.append(A), poss.append(ok & ~far), peaks.append(CL.peak_mask(A, ok, min_sep))
            A, pos, pk = np.concatenate(As), np.concatenate(poss), np.concatenate(peaks)
            ids = np.nonzero(pos)[0]                     # run order = row order
            ranked = ids[np.lexsort((ids, -A[ids]))]
            exact = ranked[:M][pk[ranked[:M]]]
            if exact.size >= k:
                rest = max(A[ranked[M]] if ranked.size > M else -np.inf, NOISE_BOUND)
                must[c] = (A[exact[k - 1]] - rest) / e > 4
        return out_r, out_s, out_sr, out_ss, must


class Column(NamedTuple):
    """One bias column as the model knows it: ``at`` fp32 [candidates] its entries at the candidates' slots; every entry of
    a live slot that is no candidate lies in [lo, hi]."""
    at: np.ndarray
    lo: float
    hi: float


def dense(L: Layout, seed=77):
    """The whole memory of a small layout on the host, by the recipe of the large one -> (bits [N, D], Sparse)."""
    import torch
    gen = torch.Generator(device="cpu").manual_seed(seed)
    cand, parts = {}, []
    for start, x, keys, tags in blocks(L, gen, "cpu"):
        cut_hoods(L, start, x, cand)
        parts.append(x.view(torch.int16).numpy().view(np.uint16).copy())
        assert np.array_equal(tags.numpy(), tag_of(L, np.arange(start, start + x.shape[0])))
    return np.concatenate(parts), Sparse(L, cand)


# ---- the cases: one table for the CPU proof and the GPU test ---------------------------------------------------------------
K, RANGE_MIN, CLIP_L, CLIP_K, CLIP_MIN = 5, 0.3, 4, 3, 0.3
MIX_W, MIX_K = [1.0, 0.5, -0.25], 5
POOL, DIV_K = 8, 4
ALL16 = tuple(range(FAMILIES))


def scope_cases(L: Layout):
    """name -> (one scope for every query, k of topk_scoped, k of topk_grouped_scoped).  k = the members of a family the
    scope holds (levels 0 and 6 share a group)."""
    s2, last = L.b2 // L.source_rows, (L.N - 1) // L.source_rows
    t = lambda r: int(tag_of(L, r))
    return {"sources above b2": (scope_of_source(s2, last), 3, 2),            # levels 0, 6 and 2
            "window across b2": ((t(L.b2 - 16), t(L.b2 + 31)), 3, 2),         # levels 4, 0 and 6
            "last rows": ((t(L.N - 16), t(L.N - 1)), 1, 1)}                   # level 2


def span_cases(L: Layout):
    """name -> (query families, spans (inclusive row ids, one per query), k)."""
    near = (12, 13, 14, 15, 0, 1, 2, 3)
    return {"across b1": (near, [(L.b1 - 4, L.b1 + 3)] * len(near), 1),       # one member each: level 1 or level 5
            "b2 to the end": (ALL16, [(L.b2 - 4, L.N - 1)] * FAMILIES, 3),    # levels 0, 6, 2
            "one per query": (ALL16, [(L.b1 + f, L.b2 + 2 * f) for f in ALL16], 4)}   # levels 5, 8, 4, 0


def mask_rows(L: Layout):
    """The planted rows around b1 and b2, both sides: six members of every family."""
    return sorted(r for r in positions(L) if abs(r - L.b1) <= HOOD or abs(r - L.b2) <= HOOD)


def clip_cases(L: Layout):
    """(start rows of the planted occurrences, which of them a source change cuts in two).  A tagged memory never matches a
    window across two sources (tests/clip_ref.py tag_breaks), and b1 and b2 begin a source: the occurrences across b2 and
    across b1 must not be found, the ones that end just below a boundary or begin at it, and the one at the tail, must."""
    return ((L.b2 - 2, L.b2 - 4, L.b2, L.b1 - 2, L.b1 - 4, L.b1, L.N - 4),
            (True, False, False, True, False, False, False))


def clips_of(L: Layout):
    plant = planted_rows(L)
    starts, _ = clip_cases(L)
    return np.stack([noisy_copy(np.stack([plant[s + i] for i in range(CLIP_L)]), 30 + c) for c, s in enumerate(starts)])


LATE_MS = 5          # the gated append's rows are tagged this many ms late: max_gap_ms below it breaks a clip across them


def fresh_rows(L: Layout, seed=99) -> np.ndarray:
    """bits [3, D]: three new directions of the first half, orthogonal to every family and to each other."""
    h = L.D // 2
    basis = base_queries(L)
    x = np.random.default_rng(seed).standard_normal((3, h))
    x, _ = np.linalg.qr((x - (x @ basis.T) @ basis).T)
    return to_bits(np.concatenate([x.T, np.zeros((3, h))], axis=1), DTYPE)


def mix_terms(L: Layout, seed=40):
    """bits [16, 3, D]: query c mixes families c, c + 1, c + 2."""
    q = [queries(L, FAMILIES, seed + j) for j in range(3)]
    return np.stack([np.stack([q[j][(c + j) % FAMILIES] for j in range(3)]) for c in ALL16])


# the biased search: column 0 boosts planted rows, column 1 is the age of every row, any other index the zero column
BIAS_K, AGE_FILL = 5, 1.0e6
BOOST = {4: 0.3, 5: 0.22}     # level 4 (0.75, just below b2) + 0.3 outranks level 0 (0.95, just above it) and level 5 (0.70,
                              # at b1 and above) + 0.22 outranks level 1 (0.90, just below b1)
BIAS_INDEX = (0, 1, 2, 0, 1, 0, 1, 0, 1, 0, 1, -1, 0, 1, 0, 1)
AGE_BETAS = (1.0, 0.3, 2.0 ** -12, 0.0)     # never negative: every entry of an age column is <= 0, so no noise row gains


def boost_rows(L: Layout):
    """(row ids, values) of ``bias_of_rows``: every family's members at the levels of BOOST."""
    pos = positions(L)
    rows = sorted(r for r, (_, j) in pos.items() if j in BOOST)
    return rows, [BOOST[pos[r][1]] for r in rows]


def age_per_ms(L: Layout) -> float:
    """The oldest row loses 0.2: the member at the tail (level 2, 0.85) then outranks the one below b1 (level 1, 0.90)."""
    return 0.2 / L.N


def bias_weights():
    """One weight per query of BIAS_INDEX: bias_ref.BETAS in turn (0.0, a negative and a tiny one among them) for the boost
    and the zero column, AGE_BETAS in turn for the age column."""
    out, seen = [], [0, 0]
    for c in BIAS_INDEX:
        pool = AGE_BETAS if c == 1 else BR.BETAS
        out.append(pool[seen[c == 1] % len(pool)])
        seen[c == 1] += 1
    return out


# the any/all search
FOLD_K, FOLD_W = 5, [1.0, 1.0, 0.9]


def fold_cases(L: Layout, seed=45):
    """op -> (terms bits [16, 3, D], weights).  ``max``: families c, c + 1, c + 2, so that every term names some of the five
    best rows; ``min``: three perturbed copies of family c - a row of family c scores about 0 against any other family, and
    so would the minimum."""
    same = np.stack([queries(L, FAMILIES, seed + j) for j in range(3)], axis=1)
    return {"max": (mix_terms(L), [FOLD_W] * FAMILIES), "min": (same, [[1.0] * 3] * FAMILIES)}


# the sequence search
SEQ_J, SEQ_G, SEQ_K, SEQ_MIN, SEQ_F = 3, 4, 3, 0.3, 3
SEQ_SEP = (SEQ_J - 1) * SEQ_G + 1         # topk_seq's default min_sep


def seq_cases(L: Layout):
    """group -> [(name, the planted chain's rows, cut: a source change lies inside it, the row its mask excludes or None)].
    One call per group (at most 8 sequences: the workspace grows with C x capacity).  b1 and b2 begin a source, so the
    chains across them are no chains on the tagged memory; the chains at gaps of 2 need max_step >= 2."""
    f = SEQ_F
    out = {}
    for name, b, gap2 in (("b2", L.b2, (L.b2 + 2 * f, L.b2 + 2 * f + 2, L.b2 + 2 * f + 4)),
                          ("b1", L.b1, (L.b1 + f, L.b1 + f + 2, L.b1 + f + 4))):
        out[name] = [(f"gaps of 2 above {name}", gap2, False, None),
                     (f"ends below {name}", (b - 3, b - 2, b - 1), False, None),
                     (f"begins at {name}", (b, b + 1, b + 2), False, None),
                     (f"across {name}", (b - 2, b - 1, b), True, None)]
    out["b2"] += [("tail", (L.N - 3, L.N - 2, L.N - 1), False, None),
                  ("control", (L.ctrl + 4, L.ctrl + 6, L.ctrl + 7), False, None),
                  # under a mask: without the chain's middle row (the families stand in the same order at every site, so
                  # the answer moves to another site), and without the row the chain steps over (the answer stays)
                  ("middle row masked", out["b2"][0][1], False, out["b2"][0][1][1]),
                  ("stepped-over row masked", out["b2"][0][1], False, out["b2"][0][1][1] - 1)]
    assert all(len(v) <= 8 for v in out.values())
    return out


def seq_steps(L: Layout, cases, seed=70):
    """bits [C, J, D]: noisy copies of each case's planted chain."""
    plant = planted_rows(L)
    return np.stack([noisy_copy(np.stack([plant[r] for r in chain]), seed + c) for c, (_, chain, _, _) in enumerate(cases)])


def seq_sel(model: Sparse, cases):
    """bool [C, candidates]: what each case's mask selects (all ones, but for the excluded row)."""
    return np.stack([np.ones(model.gid.size, bool) if x is None else model.gid != x for _, _, _, x in cases])
