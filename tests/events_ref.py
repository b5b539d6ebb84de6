"""Test oracle of the event segmentation (include/vidmem.h vm_memory_events / vm_memory_regroup_events).

``links``: the reference cosine of every row against the row before it - oracle.cref.cosine_matrix (the exact C
restatement of the reference cosine) of blocks of 16 rows against the same block shifted by one row, of which the
diagonal is read; link of the first row = 0.0.  ``opens`` is the rule of the header written out row by row; ``segment``
turns it into the outputs of vm_memory_events, ``regroup`` / ``regroup_tail`` into the key and ordinal columns a regroup
must leave.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from oracle import cref

INT64_MIN = -(1 << 63)
MS_BITS = 40
MS_MASK = (1 << MS_BITS) - 1
BLOCK = 16


def links(bits, dtype="f16") -> np.ndarray:
    """fp64 [n]: link[0] = 0.0, link[i] = reference cosine of rows i - 1 and i (uint16 bit patterns, row-id order)."""
    bits = np.ascontiguousarray(bits)
    n = bits.shape[0]
    out = np.zeros(n, np.float64)
    for a in range(1, n, BLOCK):
        b = min(n, a + BLOCK)
        m = cref.cosine_matrix(np.ascontiguousarray(bits[a - 1:b - 1]), np.ascontiguousarray(bits[a:b]), dtype=dtype)
        out[a:b] = np.diagonal(m)
    return out


def opens(link, threshold, tags=None, max_gap_ms=-1) -> np.ndarray:
    """bool [n]: row i opens an event.  Row 0 always; then !(link > threshold); then the tag clauses."""
    link = np.asarray(link, np.float64)
    n = link.size
    out = np.zeros(n, bool)
    for i in range(n):
        if i == 0 or not (link[i] > threshold):
            out[i] = True
            continue
        if tags is None:
            continue
        tp, tc = int(tags[i - 1]), int(tags[i])
        up, uc = tp == INT64_MIN, tc == INT64_MIN
        if up != uc:
            out[i] = True
        elif not up:
            step = (tc & MS_MASK) - (tp & MS_MASK)
            if (tp >> MS_BITS) != (tc >> MS_BITS) or (max_gap_ms >= 0 and (step < 0 or step > max_gap_ms)):
                out[i] = True
    return out


class Segmented(NamedTuple):
    event_of: np.ndarray      # int64 [n]
    first_rows: np.ndarray    # int64 [E] row ids
    count: int


def segment(flags, base=0) -> Segmented:
    flags = np.asarray(flags, bool)
    if flags.size == 0:
        return Segmented(np.zeros(0, np.int64), np.zeros(0, np.int64), 0)
    event_of = np.cumsum(flags).astype(np.int64) - 1
    first = base + np.nonzero(flags)[0].astype(np.int64)
    return Segmented(event_of, first, int(first.size))


def padded_first_rows(first_rows, max_events) -> np.ndarray:
    out = np.full(max_events, -1, np.int64)
    m = min(max_events, first_rows.size)
    out[:m] = first_rows[:m]
    return out


def events(bits, threshold, dtype="f16", tags=None, max_gap_ms=-1, base=0, link=None):
    """-> (links [n], Segmented) of the live rows ``bits`` (row-id order, first row id ``base``)."""
    link = links(bits, dtype) if link is None else link
    return link, segment(opens(link, threshold, tags, max_gap_ms), base)


class Regrouped(NamedTuple):
    keys: np.ndarray          # int64 [n]: the row id of each row's event's first row
    ordinals: np.ndarray      # int64 [n]
    state: tuple              # (groups, last key, open)


def regroup(flags, base=0) -> Regrouped:
    """Whole mode: what vm_memory_regroup_events leaves over the live rows."""
    seg = segment(flags, base)
    if seg.count == 0:
        return Regrouped(np.zeros(0, np.int64), np.zeros(0, np.int64), (0, 0, 0))
    keys = seg.first_rows[seg.event_of]
    return Regrouped(keys, seg.event_of, (seg.count, int(keys[-1]), 0))


def regroup_tail(keys, ordinals, flags, from_index, base=0) -> Regrouped:
    """Tail mode, from live row index ``from_index`` > 0: rows below keep ``keys`` / ``ordinals``; row from_index either
    continues its predecessor's group or opens one keyed by its own id; the rest follows.  Plain loop."""
    keys, ordinals = np.array(keys, np.int64), np.array(ordinals, np.int64)
    assert from_index > 0
    for i in range(from_index, len(flags)):
        if flags[i]:
            keys[i], ordinals[i] = base + i, ordinals[i - 1] + 1
        else:
            keys[i], ordinals[i] = keys[i - 1], ordinals[i - 1]
    return Regrouped(keys, ordinals, (int(ordinals[-1]) + 1, int(keys[-1]), 0))


def scene_flags(sizes) -> np.ndarray:
    """The flags planted scenes of these sizes should give: a flag at every scene's first row."""
    out = np.zeros(int(sum(sizes)), bool)
    out[np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)] = True
    return out


# The three planted-scene data sets of the tests: name -> (dtype, D, scenes, size seed, data seed).  Ragged scene sizes
# 1 - 23 (tests/support.group_sizes) that add up to 4864, 1808 and 3542 rows.
SETS = {"f16_768": ("f16", 768, 390, 1, 101), "bf16_1024": ("bf16", 1024, 151, 34, 102),
        "f16_128": ("f16", 128, 296, 3, 103)}


@functools.lru_cache(maxsize=None)
def dataset(name):
    """(dtype, row bits uint16 [n, D], scene sizes, links [n]) of one set: made on the CPU (the same bytes with and
    without a GPU), once per process, never modified."""
    import torch
    from tests.support import clustered, group_sizes
    dtype, D, scenes, size_seed, seed = SETS[name]
    sizes = group_sizes(scenes, "ragged", size_seed)
    rows, _ = clustered(sizes, D, dtype, seed=seed, device="cpu")
    bits = rows.contiguous().view(torch.int16).numpy().view(np.uint16)
    bits.setflags(write=False)
    link = links(bits, dtype)
    link.setflags(write=False)
    return dtype, bits, sizes, link
