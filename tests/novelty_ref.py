"""Test oracle of the novelty-gated append (include/vidmem.h vm_memory_append_novel).

Contract, in row order over a batch X[0..B) with threshold tau and what the caller knows (known_score / known_row):

    suppressor(i) = known_row[i]                     if known_row[i] >= 0 and known_score[i] > tau
                  = row_of[j], j the LOWEST j < i with keep[j] and cos(X[i], X[j]) > tau, if there is one
    keep[i]   = no suppressor
    row_of[i] = suppressor(i), or, when kept, (rows before the call) + (kept rows before i)

Two independent statements, both on oracle.cref alone (no cosine of their own):

  (A) ``gate``        the greedy rule from cref.cosine_matrix(batch, batch) plus known_*;
  (B) ``gate_loop``   one frame at a time on cref.cosine_topk(., k=1) over the memory as it grows: search, append iff
                      the best score is not above tau.

tests/test_novelty_cpu.py holds them against each other; the GPU tests compare with (A).  ``clip`` is the data recipe:
runs of 1-8 near-identical frames around random unit centres.
"""
from __future__ import annotations

import numpy as np

from oracle import cref
from tests.support import to_bits

INT64_MIN = -(1 << 63)


def clip(n: int, C: int, D: int, sigma: float, dtype: str, seed: int = 5) -> np.ndarray:
    """n rows: runs of 1-8 frames (uniform), each run around one of C random unit centres (uniform choice),
    frame = centre + sigma x N(0, 1) per component, normalised, rounded to the dtype.  -> uint16 [n, D]."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((C, D))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    out = np.empty((n, D), np.float64)
    i = 0
    while i < n:
        run = int(rng.integers(1, 9))
        c = centres[int(rng.integers(0, C))]
        for _ in range(min(run, n - i)):
            v = c + sigma * rng.standard_normal(D)
            out[i] = v / np.linalg.norm(v)
            i += 1
    return to_bits(out.astype(np.float32), dtype)


def top1(batch: np.ndarray, stored: np.ndarray, dtype: str, base: int = 0):
    """What topk(batch, 1) returns over ``stored`` (row ids base + index): (scores [B], rows [B]); nothing stored:
    rows -1."""
    B = batch.shape[0]
    if stored.shape[0] == 0:
        return np.zeros(B, np.float64), np.full(B, -1, np.int64)
    r, s = cref.cosine_topk(batch, stored, 1, dtype=dtype)
    return s[:, 0].copy(), np.where(r[:, 0] >= 0, r[:, 0] + base, -1)


def batch_matrix(batch: np.ndarray, dtype: str, threads: int = 8) -> np.ndarray:
    """cref.cosine_matrix(batch, batch); large batches in row blocks on a thread pool (ctypes releases the GIL; a
    score does not depend on the block it was computed in)."""
    B = batch.shape[0]
    if B < 1024:
        return cref.cosine_matrix(batch, batch, dtype=dtype)
    from concurrent.futures import ThreadPoolExecutor
    bounds = np.linspace(0, B, 4 * threads + 1).astype(np.int64)
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda lh: cref.cosine_matrix(batch[lh[0]:lh[1]], batch, dtype=dtype),
                            zip(bounds[:-1], bounds[1:])))
    return np.concatenate(parts)


def gate(batch: np.ndarray, tau: float, dtype: str, total: int, known_scores=None, known_rows=None):
    """(A) -> (keep bool [B], row_of int64 [B]).  ``total``: rows appended before the call."""
    B = batch.shape[0]
    keep = np.zeros(B, bool)
    row_of = np.full(B, -1, np.int64)
    if B == 0:
        return keep, row_of
    m = batch_matrix(batch, dtype)
    kept_idx = []
    for i in range(B):
        if known_rows is not None and known_rows[i] >= 0 and known_scores[i] > tau:
            row_of[i] = known_rows[i]
            continue
        sup = -1
        if kept_idx:
            close = np.nonzero(m[i, kept_idx] > tau)[0]
            if close.size:
                sup = kept_idx[int(close[0])]
        if sup >= 0:
            row_of[i] = row_of[sup]
        else:
            keep[i] = True
            row_of[i] = total + len(kept_idx)
            kept_idx.append(i)
    return keep, row_of


def gate_loop(batch: np.ndarray, tau: float, dtype: str, stored: np.ndarray):
    """(B) -> (keep bool [B], the memory afterwards uint16 [n, D]).  ``stored``: every row appended so far, in row-id
    order (no ring)."""
    rows = [r for r in stored]
    keep = np.zeros(batch.shape[0], bool)
    for i in range(batch.shape[0]):
        best = -np.inf
        if rows:
            _, s = cref.cosine_topk(batch[i:i + 1], np.stack(rows), 1, dtype=dtype)
            best = s[0, 0]
        if not best > tau:
            keep[i] = True
            rows.append(batch[i])
    D = batch.shape[1]
    return keep, (np.stack(rows) if rows else np.zeros((0, D), np.uint16))


class GatedMemory:
    """Host model of a memory under gated appends by statement (A): rows, tags and group keys in row-id order, the ring
    window, and the open-group rule of vm_memory_append_grouped over the kept rows."""

    def __init__(self, D: int, dtype: str, capacity=None):
        self.D, self.dtype, self.capacity = D, dtype, capacity
        self.rows = np.zeros((0, D), np.uint16)
        self.tags = np.zeros(0, np.int64)
        self.keys = np.zeros(0, np.int64)

    @property
    def total(self) -> int:
        return self.rows.shape[0]

    def window(self):
        """(first row id, rows) that a search sees."""
        lo = 0 if self.capacity is None else max(0, self.total - self.capacity)
        return lo, self.rows[lo:]

    def known(self, batch):
        lo, live = self.window()
        return top1(batch, live, self.dtype, base=lo)

    def append_novel(self, batch, tau, known=None, tags=None, keys=None):
        ks, kr = known if known is not None else (None, None)
        keep, row_of = gate(batch, tau, self.dtype, self.total, ks, kr)
        first = self.total
        n = int(keep.sum())
        self.rows = np.concatenate([self.rows, batch[keep]])
        t = np.full(n, INT64_MIN, np.int64) if tags is None else np.asarray(tags, np.int64)[keep]
        self.tags = np.concatenate([self.tags, t])
        k = -1 - (first + np.arange(n, dtype=np.int64)) if keys is None else np.asarray(keys, np.int64)[keep]
        self.keys = np.concatenate([self.keys, k])
        return keep, row_of
