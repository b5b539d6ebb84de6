"""Test oracle of row masks and the masked top-k (include/vidmem.h vm_topk_cosine_masked).

Contract: a mask holds one bit per physical slot, the bit of row id r being bit s & 31 of word s >> 5 with
s = r mod capacity; bits of slots without a live row are ignored.  The result of the search is the exhaustive row ranking
of vm_topk_cosine - raw reference cosines ranked by (score desc, row id asc), the score_mode mapping, the ``> min_score``
filter on the mapped score - taken over the selected live rows only, first k; -1 / 0.0 padded.  Two independent
statements:

  (A) ``masked_topk``        oracle.cref.cosine_topk (the C restatement of the reference ranking) on the selected rows
                             only, its indices mapped back to row ids: ascending index order keeps the stable tie rule;
  (B) ``masked_topk_matrix`` oracle.cref.cosine_matrix over all rows, masked, the raw scores ranked by
                             (score desc, row asc), then mapped and filtered.

tests/test_mask_cpu.py holds them against each other; the GPU tests compare with (A).  Also here: the host packing of a
row set into words, and the data and the mask sets of the scan test (tests/test_mask_gpu.py), which the CPU file needs to
prove the scan test's precondition without a GPU.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import cref
from tests.domain_ref import cert_eps  # noqa: F401  (the certificate's bound; MR.cert_eps for the tests and the other refs)
from tests.support import bits, clustered, queries_near

K, M1 = 1, 10                       # the scan test's k, and the rank M + 1 = k + 8 + 1 that bounds the rows not re-scored
QS = (1, 16, 17, 33)
SHAPES = {"n17": (17, None), "n33": (33, None), "n47": (47, None), "ring40": (57, 40)}   # rows appended, ring capacity
CLUSTERS = (5, 3, 4, 1, 2)          # cluster sizes, repeated: at most 5 rows resemble one another
FULL = 0xFFFFFFFF


def mask_words(capacity: int) -> int:
    return (capacity + 63) // 64 * 2


def pack_rows(row_ids, capacity: int) -> np.ndarray:
    """uint32 [W] with the bit of every row id set: bit s & 31 of word s >> 5, s = r mod capacity."""
    words = np.zeros(mask_words(capacity), dtype=np.uint32)
    for r in row_ids:
        s = int(r) % capacity
        words[s >> 5] |= np.uint32(1 << (s & 31))
    return words


def selected(words, base: int, n: int, capacity: int) -> np.ndarray:
    """bool [n]: which of the live rows base .. base + n - 1 a mask selects."""
    words = np.asarray(words, dtype=np.uint32)
    s = (base + np.arange(n, dtype=np.int64)) % capacity
    return ((words[s >> 5] >> (s & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def selection(masks, mask_index, Q: int, base: int, n: int, capacity: int) -> np.ndarray:
    """bool [Q, n] by vm_topk_cosine_masked's rule: no index = mask 0 for all (one mask) or mask q (Q masks); an index
    outside [0, n_masks) = the empty mask."""
    masks = np.asarray(masks, dtype=np.uint32).reshape(-1, mask_words(capacity))
    if mask_index is None:
        assert masks.shape[0] in (1, Q)
        mask_index = [0] * Q if masks.shape[0] == 1 else list(range(Q))
    out = np.zeros((Q, n), dtype=bool)
    for q, i in enumerate(mask_index):
        if 0 <= int(i) < masks.shape[0]:
            out[q] = selected(masks[int(i)], base, n, capacity)
    return out


def masked_topk(queries, rows, sel, k, dtype="f16", score_mode=0, min_score=None, base=0):
    """(A).  queries [Q,D], rows [n,D] (uint16 bit patterns) in row-id order, sel bool [Q,n] -> (rows [Q,k] int64,
    scores [Q,k] fp64); rows = base + row index."""
    queries = np.ascontiguousarray(queries)
    rows = np.ascontiguousarray(rows)
    Q = queries.shape[0]
    sel = np.asarray(sel, dtype=bool)
    assert sel.shape == (Q, rows.shape[0]), sel.shape
    out_r = np.full((Q, k), -1, np.int64)
    out_s = np.zeros((Q, k), np.float64)
    same = {}
    for q in range(Q):
        same.setdefault(sel[q].tobytes(), []).append(q)
    for qs in same.values():                # queries of one selection share one restricted memory
        idx = np.nonzero(sel[qs[0]])[0]
        if idx.size == 0:
            continue
        r, s = cref.cosine_topk(queries[qs], rows[idx], k, dtype=dtype, score_mode=score_mode, min_score=min_score)
        out_r[qs] = np.where(r >= 0, base + idx[np.maximum(r, 0)], -1)
        out_s[qs] = s
    return out_r, out_s


def masked_topk_from_scores(scores, sel, k, score_mode=0, min_score=None, base=0):
    """scores [Q,n] raw fp64 cosines in row-id order -> the masked ranking."""
    scores = np.asarray(scores, dtype=np.float64)
    Q, n = scores.shape
    out_r = np.full((Q, k), -1, np.int64)
    out_s = np.zeros((Q, k), np.float64)
    for q in range(Q):
        raw = scores[q]
        shown = (1.0 + raw) / 2.0 if score_mode == 1 else raw
        keep = np.array(sel[q], dtype=bool)
        if min_score is not None:
            keep &= shown > min_score
        cand = np.nonzero(keep)[0]
        best = cand[np.lexsort((cand, -raw[cand]))][:k]     # raw score desc, row asc
        out_r[q, :best.size] = base + best
        out_s[q, :best.size] = shown[best]
    return out_r, out_s


def masked_topk_matrix(queries, rows, sel, k, dtype="f16", score_mode=0, min_score=None, base=0):
    """(B)."""
    return masked_topk_from_scores(cref.cosine_matrix(queries, rows, dtype=dtype), sel, k, score_mode, min_score, base)


# ---- the scan test's data and masks ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_dataset(D, dtype, shape):
    """The data of the scan tests, made once on the host (tests/tile_scan_data.py uploads it): (rows, queries, base,
    oracle score matrix [33, live rows]) of one shape."""
    total, cap = SHAPES[shape]
    sizes, left = [], total
    while left:
        sizes.append(min(CLUSTERS[len(sizes) % len(CLUSTERS)], left))
        left -= sizes[-1]
    rows, _ = clustered(sizes, D, dtype, seed=D + total, device="cpu")
    base = total - cap if cap else 0
    q = queries_near(rows[base:].contiguous(), max(QS), D + total + 1, dtype)
    live = cref.cosine_matrix(bits(q), bits(rows[base:]), dtype=dtype)
    return rows, q, base, live


def host_case(D=128, dtype="f16", shape="n47"):
    """``host_dataset`` as the oracles take it: (bit patterns of the live rows, of the queries, base, score matrix)."""
    rows, q, base, live = host_dataset(D, dtype, shape)
    return bits(rows[base:]), bits(q), base, live


def mask_sets(Q: int, shape: str):
    """name -> (masks uint32 [n_masks, W], mask_index or None) of the scan test, for a memory of SHAPES[shape]: a linear
    memory whose capacity is its row count, or the ring."""
    total, cap = SHAPES[shape]
    capacity = cap or total
    n = min(total, capacity)
    W = mask_words(capacity)
    full, empty = np.full(W, FULL, dtype=np.uint32), np.zeros(W, dtype=np.uint32)
    first_tile = empty.copy()
    first_tile[0] = 0xFFFF

    def slot_bit(s):
        m = empty.copy()
        m[s >> 5] = 1 << (s & 31)
        return m
    sets = {
        "full": (full[None], None),                                   # dead and padding bits included
        "empty": (empty[None], None),
        "one_empty": (np.stack([full, empty]), [1 if i == Q // 2 else 0 for i in range(Q)]),
        "first_tile": (first_tile[None], None),                       # every other tile takes the skip path
        "alternating": (np.stack([np.full(W, 0x55555555, dtype=np.uint32), np.full(W, 0xAAAAAAAA, dtype=np.uint32)]),
                        [i % 2 for i in range(Q)]),
        "last_live": (slot_bit(n - 1)[None], None),                   # the ragged tile's last live row
        "first_dead": (slot_bit(n)[None], None),                      # slot n: the first of the padding
    }
    if cap:
        sets["newest"] = (pack_rows([total - 1], capacity)[None], None)
        sets["oldest"] = (pack_rows([total - cap], capacity)[None], None)
    return sets


def gap_ok(best_first, D) -> bool:
    """best_first: one query's exact selected scores, descending.  True when rank k and rank M + 1 are more than
    4 x cert_eps apart, or when there is no rank M + 1 (everything is re-scored exactly)."""
    return best_first.size < M1 or bool(best_first[K - 1] - best_first[M1 - 1] > 4 * cert_eps(D))


def scan_precondition(D, dtype, shape):
    """Asserts, from the oracle's scores alone, that no query of any mask set of the scan test is left to the redo."""
    _, _, base, live = host_dataset(D, dtype, shape)
    total, cap = SHAPES[shape]
    capacity = cap or total
    n = live.shape[1]
    for Q in QS:
        for name, (masks, index) in mask_sets(Q, shape).items():
            sel = selection(masks, index, Q, base, n, capacity)
            for i in range(Q):
                assert gap_ok(np.sort(live[i][sel[i]])[::-1], D), f"precondition: {shape} D={D} {dtype} {name} query {i}"
