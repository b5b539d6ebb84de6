"""GPU: two branches of what follows the tile scan in the mixed and the any/all search (csrc/topk_mix.hip: the finalize, the
redo scan, fold_terms_kernel and their launches) that no other test reaches.

1. Overflow: more rows at the cut than the candidate buffer holds, so the finalize flags the query VM_FLAG_OVERFLOW and
   the exhaustive redo answers it.  tests/test_bias_gpu.py has this for the biased search only.
2. The large-LDS launch: the terms of a query lie in dynamic LDS, J * D * 2 bytes of it, and once that and the 16 KiB
   allowed for the kernels' static arrays pass 64 KiB, the finalize, the redo scan and fold_terms_kernel are launched
   only after hipFuncSetAttribute has raised their limit.  J = 16 terms of D = 2,048 are 64 KiB, J = 13 are 52 KiB; the
   other tests stop at D = 384.

Bar: rows, fp64 score bits, the fold's winning term and the padding identical to statement (A) of tests/mix_ref.py and
tests/fold_ref.py, for the fast and the ``exact=True`` entry; flag 0 wherever the oracle's own scores say the fast path
must certify (flag0_ok: rank k and rank M + 1 more than 4 eps apart).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import cref
from tests import fold_ref as FR
from tests import mask_ref as MR
from tests import mix_ref as XR
from tests.search_checks import fold_check, mix_check
from tests.support import TD, bits, clustered, plain_memory, queries_near

pytestmark = pytest.mark.gpu


# ---- 1. overflow ----------------------------------------------------------------------------------------------------
def test_overflow_is_redone_for_the_mixed_and_the_fold_search():
    """8,192 + 300 identical rows: every row has the key of the cut, more than the 8,192 the buffer keeps."""
    from vidmem import _lib
    rows, _ = clustered([5] * 2, 128, "f16", seed=33)
    still = rows[3:4].expand(8192 + 300, -1).contiguous()
    mem = plain_memory(still, "f16")
    terms = queries_near(rows, 3, 4, "f16")[None].contiguous()                 # one query of J = 3 terms
    base, host_rows = mem.rows_host()
    assert base == 0 and host_rows.shape[0] == 8192 + 300
    w = [1.0, -0.5, 0.25]
    want = XR.mix_topk(bits(terms), [w], host_rows, None, 5)
    before = mem.mix_uncertified_count
    got_r, got_s, flags = mix_check(mem, terms, w, 5, "f16", want=want, label="8,492 equal rows")
    assert flags.tolist() == [_lib.VM_FLAG_OVERFLOW] and got_r.tolist() == [[0, 1, 2, 3, 4]]
    assert mem.mix_uncertified_count == before + 1
    same = terms[:, :1].expand(1, 3, -1).contiguous()                          # one term three times: every product ties
    for op in FR.OPS:
        want = FR.fold_topk(bits(same), [[1.0] * 3], host_rows, None, 5, op)
        assert (want[2] == 0).all()                                            # ... and the first term wins
        before = mem.fold_uncertified_count
        got_r, got_s, flags = fold_check(mem, same, [1.0] * 3, 5, op, "f16", want=want, label="8,492 equal rows")
        assert flags.tolist() == [_lib.VM_FLAG_OVERFLOW] and got_r.tolist() == [[0, 1, 2, 3, 4]]
        assert mem.fold_uncertified_count == before + 1
    mem.close()


# ---- 2. the large-LDS launch ----------------------------------------------------------------------------------------
D, CAP, TOTAL, C, K = 2048, 200, 333, 2, 5
BASE = TOTAL - CAP                                       # live rows 133 .. 332; row 200 lies in slot 0
GRADES = (0.9, 0.8, 0.7, 0.6, 0.5, 0.4)                  # cosine of a planted row with its query's centre
PLANTED = ((133, 199, 200, 260, 332, 140), (134, 201, 299, 331, 150, 175))      # live rows, the seam included
BURIED = ((50, 7), (51, 132))                            # copies of the centres that the ring has overwritten
TWINS = tuple(range(152, 176, 2))                        # twelve identical live rows at cosine 0.2 with centre 1
MIX_W = (1.0, -0.5, 0.25)                                # cycled over the J terms
FOLD_W = (1.0, 1.25, 1.5, 1.75)


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


@functools.lru_cache(maxsize=None)
def big_case(dtype, J):
    """The data, chosen on the host, and statement (A) of the three searches with and without masks, computed once.
    Query c's J terms scatter around a centre (cosine about 0.89 with it); six live rows are planted at graded cosines
    with the centre, every other row is random (cosine about +-0.02 with anything), so the five best lie far above
    rank M + 1 = 14.  Mask 0 keeps all of query 0's planted rows; mask 1 keeps two of query 1's and the twelve twins, which
    then hold ranks 3 .. 14 with one score: no certificate can part rank 5 from rank 14, the query must go to the redo."""
    rng = np.random.default_rng(2048 + J)
    centre = _unit(rng.standard_normal((C, D)))
    terms = centre[:, None, :] + 0.5 * _unit(rng.standard_normal((C, J, D)))
    rows = _unit(rng.standard_normal((TOTAL, D)))
    for c in range(C):
        for g, r in zip(GRADES, PLANTED[c]):
            rows[r] = g * centre[c] + np.sqrt(1.0 - g * g) * rows[r]
        for r in BURIED[c]:
            rows[r] = centre[c]
    rows[list(TWINS)] = 0.2 * centre[1] + np.sqrt(0.96) * rows[TWINS[0]]
    rows = torch.from_numpy(rows.astype(np.float32)).to(TD[dtype])
    terms = torch.from_numpy(terms.astype(np.float32)).to(TD[dtype]).contiguous()
    live = np.arange(BASE, TOTAL)
    keep0 = set(live[live % 3 != 1]) | set(PLANTED[0])
    keep1 = (set(live[live % 2 == 0]) - set(PLANTED[1])) | {134, 150}
    masks = np.stack([MR.pack_rows(sorted(keep0), CAP), MR.pack_rows(sorted(keep1), CAP)])
    sels = {"none": np.ones((C, CAP), dtype=bool), "masks": MR.selection(masks, None, C, BASE, CAP, CAP)}
    e = cref.cosine_matrix(bits(terms).reshape(C * J, D), bits(rows[BASE:]), dtype=dtype).reshape(C, J, CAP)
    wm = [MIX_W[j % 3] for j in range(J)]
    wf = [FOLD_W[j % 4] for j in range(J)]
    W = np.stack([XR.mix_scores_loop(e[c], wm) for c in range(C)])
    want = {"weights": {"mix": wm, "max": wf, "min": wf}}
    scores = {"mix": (W, None)}
    for op in FR.OPS:
        ft = [FR.fold_scores_loop(e[c], wf, op) for c in range(C)]
        scores[op] = (np.stack([f for f, _ in ft]), np.stack([t for _, t in ft]))
    for what, (S, T) in scores.items():
        eps = XR.eps_mix(D, XR.abs_sum(wm)) if what == "mix" else FR.eps_fold(D, FR.abs_max(wf))
        for name, sel in sels.items():
            r, s = MR.masked_topk_from_scores(S, sel, K, base=BASE)
            best = [np.sort(S[c][sel[c]])[::-1] for c in range(C)]
            M1 = XR.slack_m(K) + 1
            gap = [float(b[K - 1] - b[M1 - 1]) / eps if b.size >= M1 else np.inf for b in best]
            ok = [g > 4.0 for g in gap]                                         # flag0_ok, with the margin kept
            if what == "mix":
                assert ok == [XR.flag0_ok(b, K, D, XR.abs_sum(wm)) for b in best]
                want[what, name] = ((r, s), ok, gap)
            else:
                assert ok == [FR.flag0_ok(b, K, D, FR.abs_max(wf)) for b in best]
                want[what, name] = ((r, s, FR.terms_of_rows(T, r, BASE)), ok, gap)
    return rows, terms, masks, want


@pytest.mark.parametrize("J", [16, 13])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_terms_that_need_more_dynamic_lds_than_a_launch_gets_by_default(dtype, J):
    """J = 16: 64 KiB of terms, J = 13 (the ragged case): 52 KiB; a ring of 200 slots after 333 rows, so the live rows wrap
    and the last tile is ragged.  The oracle's scores demand flag 0 for both queries of every search without a mask and
    for query 0 under the masks; the smallest margin (rank 5 - rank 14) / eps over those, on this data, is 534 (the mixed
    search, bf16, J = 16, query 1 without a mask; the bar is 4), so no rounding of the scan decides a flag.  Query 1 under the masks has margin 0
    (the twins) and is flagged: the masked redo scan also runs from the fast entry."""
    rows, terms, masks, want = big_case(dtype, J)
    assert J * D * 2 + 16384 > 65536
    mem = plain_memory(rows.cuda(), dtype, capacity=CAP, ring=True, step=19)
    assert mem.rows_host()[0] == BASE and np.array_equal(mem.rows_host()[1], bits(rows[BASE:]))
    t = terms.cuda()
    for name in ("none", "masks"):
        m = None if name == "none" else masks
        ref, ok, gap = want["mix", name]
        assert ok == [True, name == "none"] and (name == "none" or gap[1] == 0.0), ("precondition", gap)
        got_r, _, flags = mix_check(mem, t, want["weights"]["mix"], K, dtype, m, certified=ok, want=ref,
                                    label=f"mix J={J} {name}")
        assert set(got_r[0]) <= set(PLANTED[0]) and (name == "none" or flags[1] != 0)
        for op in FR.OPS:
            ref, ok, gap = want[op, name]
            assert ok == [True, name == "none"] and (name == "none" or gap[1] == 0.0), ("precondition", op, gap)
            got_r, _, flags = fold_check(mem, t, want["weights"][op], K, op, dtype, m, certified=ok, want=ref,
                                         label=f"fold J={J} {name}")
            assert set(got_r[0]) <= set(PLANTED[0]) and (name == "none" or flags[1] != 0)
    mem.close()
