"""GPU: the three exhaustive redo scans are one kernel under three row predicates (csrc/topk_exact.hip
topk_redo_scan_kernel<DT, CHUNK, P>, csrc/vm_internal.h NoScope / TagScope / MaskScope; the grouped redo takes the same
TagScope).  The same row set said three ways - a tag range, the mask of that range, the range on a memory whose every row
is its own group - must give the same rows and the same fp64 score bits, and all three the oracle's (tests/scope_ref.py,
statement (A)).  No tolerance: the bar is bit identity.

Memory: a tagged, grouped RING of capacity 200 (not a multiple of 16) after 333 rows, so it has wrapped: rows 133 .. 332
live, row 200 in slot 0.  D = 128, tag = row id, one group per row.  Q = 17 (two query tiles, the second ragged), k = 5.
Scopes: per query a window over the seam between slot 199 and slot 0, one of them reaching below the oldest live row, and
one empty scope.
"""
import numpy as np
import pytest
import torch

from tests import scope_ref as S
from tests.support import bits

pytestmark = pytest.mark.gpu

CAP, TOTAL, D, Q, K = 200, 333, 128, 17, 5
ALL = (S.INT64_MIN, S.INT64_MAX)


def _bits64(t):
    return t.cpu().numpy().view(np.int64)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_tag_range_mask_and_one_row_groups_agree_bit_for_bit(dtype):
    from vidmem.memory import EmbeddingMemory
    td = torch.float16 if dtype == "f16" else torch.bfloat16
    g = torch.Generator("cuda").manual_seed(41)
    rows = torch.randn(TOTAL, D, device="cuda", generator=g).to(td)
    ids = torch.arange(TOTAL, device="cuda", dtype=torch.int64)
    mem = EmbeddingMemory(CAP, D, dtype, ring=True, grouped=True, tagged=True)
    for c0 in range(0, TOTAL, 111):          # three appends; the last one wraps
        mem.append(rows[c0:c0 + 111], group=ids[c0:c0 + 111], tag=ids[c0:c0 + 111])
    base, host_rows = mem.rows_host()
    assert base == TOTAL - CAP and host_rows.shape[0] == CAP
    tags = np.arange(base, TOTAL, dtype=np.int64)
    pick = torch.arange(Q, device="cuda") * 11 + base + 3
    q = (rows[pick].float() + 0.05 * torch.randn(Q, D, device="cuda", generator=g)).to(td)

    # row 199 sits in the last slot, row 200 in slot 0: every window holds both
    scopes = [(183 + q_, 204 + 3 * q_) for q_ in range(Q)]
    scopes[4] = (100, 215)                   # from below the oldest live row (133): the dead ids select nothing
    scopes[9] = (250, 249)                   # empty
    for lo, hi in scopes[:9] + scopes[10:]:
        assert lo <= 199 and hi >= 200
    want_r, want_s = S.scoped_topk(bits(q), host_rows, tags, scopes, K, dtype=dtype, base=base)
    assert (want_r[9] == -1).all() and (np.delete(want_r, 9, axis=0) >= 0).all()

    sc = torch.tensor(scopes, dtype=torch.int64, device="cuda")
    masks = torch.stack([mem.mask_of_scope(s) for s in scopes])      # mask q for query q
    s_tag, r_tag = mem.topk_scoped(q, K, sc, exact=True)
    s_msk, r_msk = mem.topk_masked(q, K, masks, exact=True)
    s_grp, r_grp, k_grp = mem.topk_grouped_scoped(q, K, sc, exact=True)
    for name, s, r in (("scoped", s_tag, r_tag), ("masked", s_msk, r_msk), ("grouped scoped", s_grp, r_grp)):
        assert np.array_equal(r.cpu().numpy(), want_r), (name, r.cpu().numpy()[:3], want_r[:3])
        assert np.array_equal(_bits64(s), want_s.view(np.int64)), f"{name}: score bits differ from the oracle"
    assert torch.equal(k_grp, r_grp)         # the group key of a row is its id; -1 where there is no hit

    # no predicate against the predicate that admits every row
    s_all, r_all = mem.topk(q, K, exact=True)
    s_sc, r_sc = mem.topk_scoped(q, K, ALL, exact=True)
    s_mk, r_mk = mem.topk_masked(q, K, ~mem.new_mask(), exact=True)
    for s, r in ((s_sc, r_sc), (s_mk, r_mk)):
        assert torch.equal(r_all, r) and np.array_equal(_bits64(s_all), _bits64(s))
    want_r, want_s = S.scoped_topk(bits(q), host_rows, tags, ALL, K, dtype=dtype, base=base)
    assert np.array_equal(r_all.cpu().numpy(), want_r) and np.array_equal(_bits64(s_all), want_s.view(np.int64))
    mem.close()
