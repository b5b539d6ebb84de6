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
import numpy as np
import pytest

from tests import group_ref as G
from tests import range_ref as R
from tests import scope_ref as S
from tests.search_checks import range_check
from tests.support import grouped_memory, tagged_memory
from tests.tile_scan_data import K, QS, SHAPES, dataset, gap_ok, scope_sets, tags_of

pytestmark = pytest.mark.gpu

TAU = 0.29                          # range threshold: between the cross-cluster and the in-cluster scores


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
