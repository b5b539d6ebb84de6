"""GPU: the shared fp32 tile scan (csrc/topk_tile_scan.h) where its common text can go wrong, through the three searches
that run it: grouped top-k, scoped top-k and the range search.

Shapes: D = 128 and 384 are 4 and 12 k-steps (less than one load batch of 8, and one and a half); 17, 33 and 47 live rows
are one, two and three 16-row tiles with a ragged last one; a ring of capacity 40 after 57 rows has its head in slot 17;
Q = 1, 16, 17, 33 are one 16-query tile, the switch to two, and a second query group with one live query.  k = 1, so the
searches re-score M = 9 candidates and the certificate bounds the 10th against the rest.

Bar: rows and fp64 score bits identical to the refs (tests/group_ref.py, tests/scope_ref.py, tests/range_ref.py over one
oracle score matrix per data set), for the fast and the exhaustive entries.  The exhaustive redo would hide a broken
scan, so the fast entries must also answer alone: every per-query flag 0 (grouped, scoped), out_rescored == out_counts
(range).  That is a demand on the data first, asserted from the oracle's fp64 scores before any GPU call: each query's
best and 10th exact in-scope score (group maxima for grouped) lie more than 4 x cert_eps(D) apart, and no exact score
lies within 4 x cert_eps(D) of the range threshold.  The certificate needs 2 x.
"""
import functools

import numpy as np
import pytest
import torch

from tests import group_ref as G
from tests import range_ref as R
from tests import scope_ref as S
from tests.test_group_topk_gpu import _bits, clustered, grouped_memory, queries_near
from tests.test_range_gpu import check as range_check
from tests.test_scope_topk_gpu import ALL, make_tag, tagged_memory

pytestmark = pytest.mark.gpu

K, M1 = 1, 10                       # k, and the rank M + 1 = k + 8 + 1 that bounds the rows not re-scored
TAU = 0.29                          # range threshold: between the cross-cluster and the in-cluster scores
QS = (1, 16, 17, 33)
SHAPES = {"n17": (17, None), "n33": (33, None), "n47": (47, None), "ring40": (57, 40)}   # rows appended, ring capacity
CLUSTERS = (5, 3, 4, 1, 2)          # cluster sizes, repeated: at most 5 rows resemble one another


@functools.lru_cache(maxsize=None)
def dataset(D, dtype, shape):
    """(rows, queries, base, oracle score matrix [33, live rows]) of one shape, made once on the host."""
    total, cap = SHAPES[shape]
    sizes, left = [], total
    while left:
        sizes.append(min(CLUSTERS[len(sizes) % len(CLUSTERS)], left))
        left -= sizes[-1]
    rows, _ = clustered(sizes, D, dtype, seed=D + total, device="cpu")
    base = total - cap if cap else 0
    q = queries_near(rows[base:].contiguous(), max(QS), D + total + 1, dtype)
    live = R.cref.cosine_matrix(_bits(q), _bits(rows[base:]), dtype=dtype)
    return rows.cuda(), q.cuda(), base, live


def tags_of(total):
    """Two sources interleaved row by row: tag = (row id % 2) << 40 | row id."""
    r = np.arange(total, dtype=np.int64)
    return ((r % 2) << 40) | r


def scope_sets(Q, base, cap):
    """name -> Q scopes.  `first_tile`: source 0's rows of physical slots 0 .. 15 - every other tile has no in-scope
    row and takes the skip path."""
    r0 = cap if cap else 0          # the row id in physical slot 0 (a ring of capacity cap after cap + 17 rows: cap)
    return {"all": [ALL] * Q,
            "half_per_query": [(make_tag(i % 2, 0), make_tag(i % 2, (1 << 40) - 1)) for i in range(Q)],
            "one_empty": [(10, 5) if i == Q // 2 else ALL for i in range(Q)],
            "first_tile": [(make_tag(0, r0), make_tag(0, r0 + 15))] * Q}


def gap_ok(best_first, D):
    """best_first: one query's exact scores, descending.  True when rank k and rank M + 1 are more than 4 x cert_eps
    apart, or when there is no rank M + 1 (everything is re-scored exactly)."""
    return best_first.size < M1 or best_first[K - 1] - best_first[M1 - 1] > 4 * R.cert_eps(D)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("D,dtype", [(128, "f16"), (128, "bf16"), (384, "f16"), (384, "bf16")])
def test_scoped_and_range(D, dtype, shape):
    rows, q_all, base, live = dataset(D, dtype, shape)
    total, cap = SHAPES[shape]
    tags = tags_of(total)
    mem = tagged_memory(rows, tags, dtype, capacity=cap, ring=cap is not None, step=19)
    assert mem.rows_host()[0] == base and np.array_equal(mem.tags_host(), tags[base:])
    near = np.abs(live - TAU).min()
    print(f"{shape} D={D} {dtype}: nearest score to {TAU} is {near / R.cert_eps(D):.0f} x cert_eps away")
    assert near > 4 * R.cert_eps(D), "precondition: an exact score lies within 4 x cert_eps of the threshold"
    for Q in QS:
        q = q_all[:Q].contiguous()
        counts, resc = range_check(mem, q, TAU, R.range_from_scores(live[:Q], TAU, base=base), label=f"{shape} Q={Q}")
        assert counts.sum() > 0 and np.array_equal(resc, counts), (Q, resc[:8], counts[:8])
        for name, scopes in scope_sets(Q, base, cap).items():
            lo, hi = S.scope_arrays(scopes, Q)
            for i in range(Q):          # precondition of flag 0, from the oracle's scores alone
                inside = live[i][S.scope_mask(tags[base:], lo[i], hi[i])]
                assert gap_ok(np.sort(inside)[::-1], D), f"precondition: {shape} {name} query {i}"
            want_r, want_s = S.scoped_topk_from_scores(live[:Q], tags[base:], scopes, K, base=base)
            for exact in (False, True):
                s, r = mem.topk_scoped(q, K, scopes, exact=exact)
                assert np.array_equal(r.cpu().numpy(), want_r), (name, Q, exact)
                assert np.array_equal(s.cpu().numpy().view(np.int64), want_s.view(np.int64)), (name, Q, exact)
                if not exact:
                    flags = mem.last_scope_flags[:Q].cpu().numpy()
                    assert (flags == 0).all(), f"{shape} {name} Q={Q}: the scan left queries to the redo: {flags}"
            want = R.range_from_scores(live[:Q], TAU, tags=tags[base:], scopes=scopes, base=base)
            counts, resc = range_check(mem, q, TAU, want, scopes=scopes, label=f"{shape} {name} Q={Q}")
            assert np.array_equal(resc, counts), (name, Q, resc[:8], counts[:8])
            if name == "one_empty":
                assert counts[Q // 2] == 0 and want_r[Q // 2, 0] == -1
    mem.close()


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("D,dtype", [(128, "f16"), (128, "bf16"), (384, "f16"), (384, "bf16")])
def test_grouped(D, dtype, shape):
    rows, q_all, base, live = dataset(D, dtype, shape)
    total, cap = SHAPES[shape]
    for size in (1, 3):                 # groups of 3 cross the lanes' 4-row runs and the 16-row tiles
        sizes = [size] * (total // size) + ([total % size] if total % size else [])
        mem = grouped_memory(rows, sizes, dtype, capacity=cap, ring=cap is not None)
        keys = mem.group_keys_host()
        gid = G.group_ids(keys)
        assert mem.rows_host()[0] == base and gid[-1] + 1 == len(sizes) - base // size
        for i in range(max(QS)):        # precondition of flag 0: the exact group maxima
            maxima = np.array([live[i][gid == g].max() for g in range(gid[-1] + 1)])
            assert gap_ok(np.sort(maxima)[::-1], D), f"precondition: {shape} groups of {size} query {i}"
        for Q in QS:
            q = q_all[:Q].contiguous()
            want_r, want_s, want_k = G.grouped_topk_from_scores(live[:Q], keys, K, base=base)
            for exact in (False, True):
                s, r, kk = mem.topk_grouped(q, K, exact=exact)
                assert np.array_equal(r.cpu().numpy(), want_r), (size, Q, exact)
                assert np.array_equal(kk.cpu().numpy(), want_k), (size, Q, exact)
                assert np.array_equal(s.cpu().numpy().view(np.int64), want_s.view(np.int64)), (size, Q, exact)
                if not exact:
                    flags = mem.last_group_flags[:Q].cpu().numpy()
                    assert (flags == 0).all(), f"{shape} groups of {size} Q={Q}: queries left to the redo: {flags}"
        mem.close()
