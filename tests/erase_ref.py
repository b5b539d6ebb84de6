"""CPU model of erase (include/vidmem.h vm_memory_erase_scoped / vm_memory_erase_rows), numpy only.

Contract: given the columns of a memory in row-id order and a drop mask, the memory afterwards holds the survivors in
their old order, renumbered 0 .. n'-1; ``new_row_of`` maps every old id to its new one, -1 for an erased row.  Groups
follow the header's definition, a maximal run of equal keys, taken over the SURVIVORS: two groups with one key that
become adjacent are one group.  The group state is that of a fresh memory after one grouped append of the survivors:
(groups opened, last key, open) = (number of runs, the last survivor's key, 1), or (0, 0, 0) when nothing is left.

Search expectations over the survivors come from tests/topk_ref.py, group_ref.py, scope_ref.py and the C oracle: the
cosine and the ranking are not defined here.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np


class Columns(NamedTuple):
    rows: np.ndarray                   # uint16 [n, D] bit patterns
    tags: Optional[np.ndarray]         # int64 [n] or None
    keys: Optional[np.ndarray]         # int64 [n] or None


class ErasedModel(NamedTuple):
    cols: Columns                      # the survivors
    new_row_of: np.ndarray             # int64 [n_old]
    count: int                         # rows erased
    ordinals: Optional[np.ndarray]     # int64 [n'] group ordinal of every survivor (grouped memories)
    state: Optional[tuple]             # (groups, last key, open)


def mask_of_scopes(tags, scopes) -> np.ndarray:
    """Drop mask of the scoped form: the tag lies in at least one inclusive range; lo > hi matches nothing."""
    tags = np.asarray(tags, dtype=np.int64)
    sc = np.asarray(scopes, dtype=np.int64).reshape(-1, 2)
    drop = np.zeros(tags.shape[0], bool)
    for lo, hi in sc:
        drop |= (tags >= lo) & (tags <= hi)
    return drop


def mask_of_rows(n, ids) -> np.ndarray:
    """Drop mask of the rows form: ids < 0 or >= n are ignored, duplicates allowed, any shape."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    drop = np.zeros(n, bool)
    drop[ids[(ids >= 0) & (ids < n)]] = True
    return drop


def ordinals_of(keys) -> np.ndarray:
    """Group ordinal of every row: runs of equal consecutive keys, counted from 0."""
    keys = np.asarray(keys, dtype=np.int64)
    if keys.size == 0:
        return np.zeros(0, np.int64)
    return np.concatenate([[0], np.cumsum(keys[1:] != keys[:-1])]).astype(np.int64)


def erase(cols: Columns, drop) -> ErasedModel:
    drop = np.asarray(drop, dtype=bool)
    n = cols.rows.shape[0]
    assert drop.shape == (n,)
    keep = ~drop
    new_row_of = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64)
    out = Columns(cols.rows[keep], None if cols.tags is None else np.asarray(cols.tags, np.int64)[keep],
                  None if cols.keys is None else np.asarray(cols.keys, np.int64)[keep])
    ordinals = state = None
    if out.keys is not None:
        ordinals = ordinals_of(out.keys)
        state = (int(ordinals[-1]) + 1, int(out.keys[-1]), 1) if out.keys.size else (0, 0, 0)
    return ErasedModel(out, new_row_of, int(drop.sum()), ordinals, state)


def compose(first: np.ndarray, second: np.ndarray) -> np.ndarray:
    """The id map of two erases in a row: old id -> id after the first -> id after the second."""
    first = np.asarray(first, np.int64)
    return np.where(first >= 0, np.asarray(second, np.int64)[np.maximum(first, 0)], -1).astype(np.int64)
