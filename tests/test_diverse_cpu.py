"""No GPU: the diverse top-k oracle against itself and against the row oracle, the host half of the feature (the Python
refusals, the scratch owner rule, the header), and the two preconditions of the GPU scan test (tests/test_diverse_gpu.py)
proven from oracle scores alone.
"""
import os
import re

import numpy as np
import pytest
import torch

from oracle import cref
from tests import diverse_ref as DR
from tests import mask_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_case = MR.host_case


def _same(a, b):
    return np.array_equal(a[0], b[0]) and all(np.array_equal(x.view(np.int64), y.view(np.int64))
                                              for x, y in zip(a[1:], b[1:]))


# ---- the oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype", DR.DTS)
def test_loop_and_array_statements_agree_bit_for_bit(D, dtype):
    rows, q, base, live = _case(D, dtype, "ring40")
    Q = 12
    q, live = q[:Q], live[:Q]
    sels = DR.scan_selections(Q, "ring40", base, rows.shape[0])
    sim = DR.sim_matrix(rows, dtype)
    for name in ("none", "alternating", "first_tile", "one_empty"):
        sel = sels[name][2]
        for k, pool in DR.K_POOL:
            for lam in (*DR.LAMS, DR.lam_vector(Q), -0.5, 1.5):     # outside [0, 1]: still the formula
                a = DR.diverse_topk(q, rows, sel, k, pool, lam, dtype, base=base, sim=sim)
                b = DR.diverse_topk_arrays(q, rows, sel, k, pool, lam, dtype, base=base, scores=live, sim=sim)
                assert _same(a, b), (name, k, pool, lam)
    # the pairs scored for the pool alone are the pairs of the whole matrix
    assert _same(DR.diverse_topk(q, rows, None, 5, 16, 0.5, dtype, base=base),
                 DR.diverse_topk(q, rows, None, 5, 16, 0.5, dtype, base=base, sim=sim))
    a = DR.diverse_topk(q, rows, None, 5, 16, 0.5, dtype, min_score=0.1, base=base)
    assert _same(a, DR.diverse_topk_arrays(q, rows, None, 5, 16, 0.5, dtype, min_score=0.1, base=base))
    assert (a[1][a[0] >= 0] > 0.1).all()


@pytest.mark.parametrize("D,dtype", DR.DTS)
@pytest.mark.parametrize("shape", list(MR.SHAPES))
def test_sim_is_bit_symmetric(D, dtype, shape):
    rows, _, _, _ = _case(D, dtype, shape)
    S = DR.sim_matrix(rows, dtype)
    assert np.array_equal(S.view(np.int64), S.T.view(np.int64))
    assert not np.signbit(S[S == 0.0]).any()                        # a sum that starts at +0.0 never ends at -0.0


@pytest.mark.parametrize("D,dtype", DR.DTS)
def test_lam_one_is_the_row_oracle_whatever_the_pool(D, dtype):
    rows, q, base, live = _case(D, dtype)
    sim = DR.sim_matrix(rows, dtype)
    for k in (1, 5, 20):
        for cut in (None, 0.2, -0.1):
            r, s = cref.cosine_topk(q, rows, k, dtype=dtype, min_score=cut)
            for pool in (k, 2 * k, 64):
                gr, gs, gv = DR.diverse_topk(q, rows, None, k, pool, 1.0, dtype, min_score=cut, sim=sim)
                assert np.array_equal(gr, r) and np.array_equal(gs.view(np.int64), s.view(np.int64)), (k, cut, pool)
                assert np.array_equal(gv.view(np.int64), s.view(np.int64))           # 1.0 * e - 0.0 * red = e
    sel = DR.scan_selections(33, "n47", base, 47)["alternating"][2]
    r, s = MR.masked_topk(q, rows, sel, 5, dtype=dtype)
    gr, gs, _ = DR.diverse_topk(q, rows, sel, 5, 16, 1.0, dtype)
    assert np.array_equal(gr, r) and np.array_equal(gs.view(np.int64), s.view(np.int64))


def test_pool_equal_to_k_permutes_the_top_k():
    rows, q, base, live = _case(384, "f16")
    for k in (5, 17):
        r, s = cref.cosine_topk(q, rows, k, dtype="f16")
        for lam in (0.0, 0.5):
            gr, gs, _ = DR.diverse_topk(q, rows, None, k, k, lam, "f16")
            assert np.array_equal(np.sort(gr, axis=1), np.sort(r, axis=1))
            assert np.array_equal(gr[:, 0], r[:, 0])                # step 0 is the best row by definition
            for i in range(gr.shape[0]):                            # every pick carries its own relevance
                assert {(int(a), float(b)) for a, b in zip(gr[i], gs[i])} == {(int(a), float(b)) for a, b in zip(r[i], s[i])}
        assert (gr != r).any()


def test_permuting_the_queries_permutes_the_results():
    rows, q, base, live = _case()
    lam = DR.lam_vector(33)
    sel = DR.scan_selections(33, "n47", base, 47)["alternating"][2]
    a = DR.diverse_topk(q, rows, sel, 5, 16, lam, base=base)
    perm = np.random.default_rng(5).permutation(33)
    b = DR.diverse_topk(q[perm], rows, sel[perm], 5, 16, [lam[i] for i in perm], base=base)
    assert _same(b, tuple(x[perm] for x in a))


def test_a_pool_larger_than_the_selected_rows_pads():
    rows, q, base, live = _case(128, "bf16", "n17")
    r, s, v = DR.diverse_topk(q[:4], rows, None, 64, 64, 0.5, "bf16")
    assert (r[:, :17] >= 0).all() and (r[:, 17:] == -1).all() and (s[:, 17:] == 0.0).all() and (v[:, 17:] == 0.0).all()
    assert all(sorted(x[:17].tolist()) == list(range(17)) for x in r)
    sel = np.zeros((4, 17), dtype=bool)
    sel[:, 3] = True
    r, s, v = DR.diverse_topk(q[:4], rows, sel, 5, 8, 0.5, "bf16")
    assert r.tolist() == [[3, -1, -1, -1, -1]] * 4
    r, s, v = DR.diverse_topk(q[:4], rows, ~sel & False, 5, 8, 0.5, "bf16")
    assert (r == -1).all() and (s == 0.0).all() and (v == 0.0).all()


# ---- the Python layer, before the library is called ------------------------------------------------------------------------
def test_python_refusals_and_scratch():
    from tests.host_memory import host_memory
    from tests.host_memory import SizingLibrary
    from vidmem import memory as M
    mem = host_memory(capacity=100)
    q = torch.zeros((2, mem.dim))
    for k in (0, 65):
        with pytest.raises(ValueError, match="k"):
            mem.topk_diverse(q, k)
    with pytest.raises(ValueError, match="pool <= 64"):
        mem.topk_diverse(q, 5, pool=65)
    with pytest.raises(ValueError, match="k <= pool"):
        mem.topk_diverse(q, 5, pool=4)
    for lam in (-0.1, 1.5, float("nan"), float("inf"), [0.5, 2.0], torch.tensor([0.5, -1.0], dtype=torch.float64)):
        with pytest.raises(ValueError, match="lam must lie"):
            mem.topk_diverse(q, 5, lam=lam)
    with pytest.raises(ValueError, match="values of lam"):
        mem.topk_diverse(q, 5, lam=[0.5, 0.5, 0.5])
    with pytest.raises(ValueError, match="dimension"):
        mem.topk_diverse(torch.zeros((2, mem.dim + 1)), 5)
    with pytest.raises(ValueError, match="width"):
        mem.topk_diverse(q, 3, mask=torch.zeros(mem.mask_words + 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="mask_index"):
        mem.topk_diverse(q, 3, mask=torch.zeros((3, mem.mask_words), dtype=torch.int32))
    with pytest.raises(ValueError, match="needs a mask"):
        mem.topk_diverse(q, 3, mask_index=[0, 0])
    with pytest.raises(ValueError, match="NaN"):
        mem.topk_diverse(q, 3, min_score=float("nan"))
    with pytest.raises(ValueError, match="k <= pool"):
        mem.prepare_topk_diverse(1, 9, 8)
    assert M.EmbeddingMemory._diverse_pool(3, None) == (3, 12) and M.EmbeddingMemory._diverse_pool(40, None) == (40, 64)
    assert M.EmbeddingMemory._diverse_pool(64, None) == (64, 64) and M.EmbeddingMemory._diverse_pool(7, 7) == (7, 7)
    sized = host_memory(capacity=16, library=SizingLibrary())
    first = sized.prepare_topk_diverse(4, 5, 16)                    # the stand-in sizes any vm_*_workspace_bytes entry
    assert isinstance(first, M.DiverseTopkScratch) and first.fits(sized, 4, 16)
    assert first.flags.dtype == torch.int32 and first.mmr.dtype == torch.float64 and first.mmr.numel() == 4 * 16
    assert sized.prepare_topk_diverse(4, 16, 16) is first           # k does not size the workspace
    assert sized.prepare_topk_diverse(2, 2) is first                # pool 8 fits the buffers of pool 16
    assert sized.prepare_topk_diverse(64, 3, 32) is not first       # replaced, never resized
    small = M.DiverseTopkScratch.for_(sized, 1, 4)
    with pytest.raises(ValueError, match="caller-owned"):
        sized.topk_diverse(torch.zeros((2, sized.dim)), 2, pool=8, scratch=small)
    assert mem.last_diverse_flags is None and mem.last_diverse_mmr is None and mem.diverse_uncertified_count == 0


def test_header_and_library():
    from vidmem import _lib
    text = open(os.path.join(ROOT, "include", "vidmem.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("1 <= k <= pool <= 64",
                   "lam: device fp64 [Q]",
                   "mu = 1.0 - lam",
                   "v_i = (lam * e_i) - (mu * red_i)",
                   "with one rounding per operation, never fused",
                   "ties - -0.0 against +0.0 included - go to the smaller row id",
                   "which is symmetric bit for bit",
                   "lam = 1.0 gives the rows and scores of vm_topk_cosine (or _masked), first k, bit for bit, whatever the pool",
                   "pool == k only reorders the top k",
                   "not on the other queries of the call",
                   "VM_ERR_NOMEM for a workspace below vm_topk_diverse_workspace_bytes",
                   "with the outputs untouched"):
        assert phrase in flat, phrase
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for decl in (r"size_t vm_topk_diverse_workspace_bytes\(const vm_memory \*mem, int Q, int pool\);",
                 r"int vm_topk_cosine_diverse\(vm_memory \*mem, const void \*queries, int Q, int k, int pool, "
                 r"const double \*lam,",
                 r"int vm_topk_cosine_diverse_exact\(vm_memory \*mem, const void \*queries, int Q, int k, int pool, "
                 r"const double \*lam,"):
        assert re.search(decl, code), decl
    L = _lib.lib()
    assert L.vm_abi_version() == 4
    for sym in ("vm_topk_diverse_workspace_bytes", "vm_topk_cosine_diverse", "vm_topk_cosine_diverse_exact"):
        assert sym in _lib.SYMBOLS
        getattr(L, sym)
    assert L.vm_topk_diverse_workspace_bytes(None, 1, 1) == 0
    assert L.vm_topk_cosine_diverse(None, None, 1, 1, 1, None, None, 0, None, 0, 0.0, 1, 0, None, None, None, None, None,
                                    None, 0, None) == _lib.VM_ERR_INVALID
    assert L.vm_topk_cosine_diverse_exact(None, None, 1, 1, 1, None, None, 0, None, 0, 0.0, 1, 0, None, None, None, None,
                                          0, None) == _lib.VM_ERR_INVALID


# ---- the GPU scan test's preconditions -------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype", DR.DTS)
def test_scan_preconditions(D, dtype):
    """(i) Without a mask no query of the scan test is left to the redo: at k = pool, rank ``pool`` and rank M + 1 of the
    oracle's scores are more than 4 x cert_eps(D) apart, or fewer than M + 1 rows are live.  (ii) The test is not vacuous:
    at lam = 0.5, k = 5 the picks differ from plain top-5 for at least half of the 33 queries of every shape and pool."""
    for shape in MR.SHAPES:
        rows, q, base, live = _case(D, dtype, shape)
        sim = DR.sim_matrix(rows, dtype)
        for pool in sorted({p for _, p in DR.K_POOL} | set(DR.POOLS)):
            for i in range(33):
                assert DR.flag0_ok(np.sort(live[i])[::-1], pool, D), f"(i): {shape} D={D} {dtype} pool={pool} query {i}"
        top5, _ = cref.cosine_topk(q, rows, 5, dtype=dtype)
        for pool in DR.POOLS:
            picked, _, _ = DR.diverse_topk(q, rows, None, 5, pool, 0.5, dtype, sim=sim)
            differ = int((picked != top5).any(axis=1).sum())
            assert 2 * differ >= 33, f"(ii): {shape} D={D} {dtype} pool={pool}: {differ} of 33"
