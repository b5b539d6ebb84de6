"""No GPU: the biased top-k's oracle against itself and against the row oracle, the two facts behind the zero-bias
identity, the bound restated and checked numerically, the host half of the feature (the Python refusals, the scratch
owner rule, the header), planted defects that statement (A) must catch on the scan test's own data, and the precondition
of the GPU scan test (tests/test_bias_gpu.py) proven from oracle scores alone.
"""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import cref
from tests import bias_ref as BR
from tests import mask_ref as MR
from tests.support import same_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(D=128, dtype="f16", shape="n47"):
    total, cap = MR.SHAPES[shape]
    return (*MR.host_case(D, dtype, shape), cap or total)


def _bits64(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


# ---- the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype", BR.DTS)
def test_loop_and_array_statements_agree_bit_for_bit(D, dtype):
    for shape in MR.SHAPES:
        rows, q, base, live, cap = _case(D, dtype, shape)
        n = live.shape[1]
        cols = BR.set_columns(base, n, cap)
        for si in range(len(BR.SETS)):
            b = BR.row_bias(cols[si:si + 1], None, 1, base, n, cap)[0]
            for beta in BR.BETAS + (-2.0 ** 20, 1.0 / 3):
                for qi in (0, 16, 32):
                    a, c = BR.bias_scores_loop(live[qi], beta, b), BR.bias_scores(live[qi], beta, b)
                    assert np.array_equal(_bits64(a), _bits64(c)), (shape, si, beta, qi)
    rows, q, base, live, cap = _case(D, dtype, "ring40")
    cols = BR.set_columns(base, live.shape[1], cap)
    index = [BR.query_case(i)[0] for i in range(33)]
    betas = [BR.query_case(i)[1] for i in range(33)]
    sel = MR.selection(*MR.mask_sets(33, "ring40")["alternating"], 33, base, rows.shape[0], cap)
    for k in (1, 5, 64):
        assert same_arrays(BR.bias_topk(q, rows, cols, index, betas, sel, k, dtype, base=base, capacity=cap),
                     BR.bias_topk(q, rows, cols, index, betas, sel, k, dtype, base=base, capacity=cap,
                                  scores=BR.bias_scores))


@pytest.mark.parametrize("D,dtype", BR.DTS)
def test_zero_weight_and_zero_column_are_the_row_oracle(D, dtype):
    rows, q, base, live, cap = _case(D, dtype)
    n = rows.shape[0]
    cols = BR.set_columns(base, n, cap)
    q4 = q[:4]
    zero_col, big_col = cols[0:1], cols[4:5]
    for k in (1, 5, 20):
        for cut in (None, 0.2, -0.1):
            want = cref.cosine_topk(q4, rows, k, dtype=dtype, min_score=cut)
            for beta in (0.0, -0.0):                                # beta = 0: whatever the column holds
                got = BR.bias_topk(q4, rows, big_col, None, [beta] * 4, None, k, dtype, min_score=cut, capacity=cap)
                assert same_arrays(got, want), (k, cut, beta)
            for beta in (1.0, -0.5, 2.0 ** 20):                     # a column of zeros: whatever the weight
                got = BR.bias_topk(q4, rows, zero_col, None, [beta] * 4, None, k, dtype, min_score=cut, capacity=cap)
                assert same_arrays(got, want), (k, cut, beta)
            got = BR.bias_topk(q4, rows, big_col, [7, -1, 1, 5], None, None, k, dtype, min_score=cut, capacity=cap)
            assert same_arrays(got, want), "an index outside [0, n_bias) is the zero column"
        masks, index = MR.mask_sets(4, "n47")["alternating"]
        sel = MR.selection(masks, index, 4, base, n, cap)
        want = MR.masked_topk(q4, rows, sel, k, dtype=dtype, base=base)
        assert same_arrays(BR.bias_topk(q4, rows, big_col, None, [0.0] * 4, sel, k, dtype, base=base, capacity=cap), want)
        assert same_arrays(BR.bias_topk(q4, rows, zero_col, None, [0.3] * 4, sel, k, dtype, base=base, capacity=cap), want)


def test_the_reference_cosine_is_never_minus_zero_and_adding_a_zero_changes_no_other_value():
    """The two facts behind the identity "beta = 0 or a column of zeros is vm_topk_cosine bit for bit":
    (1) the reference cosine is never -0.0: its dot product starts at +0.0, and +0.0 + (-0.0) = +0.0 in round to nearest,
        so a sum of products that are all +-0.0 is +0.0; a zero norm gives the literal 0.0; +0.0 / positive = +0.0;
    (2) e + (+-0.0) = e bit for bit for every e other than -0.0 (and beta * 0.0 is +-0.0 for every finite beta)."""
    # (1) on every data set of the scan test ...
    seen_zero = False
    values = []
    for D, dtype in BR.DTS:
        for shape in MR.SHAPES:
            live = MR.host_dataset(D, dtype, shape)[3]
            assert not np.signbit(live[live == 0.0]).any(), (D, dtype, shape)
            values.append(live.ravel())
    # ... and where a -0.0 could arise: every product is -0.0 or +0.0, a zero row, a zero query
    one = np.float16(1.0).view(np.uint16)
    neg = np.float16(-1.0).view(np.uint16)
    mz = np.float16(-0.0).view(np.uint16)
    qv = np.zeros((3, 128), dtype=np.uint16)
    qv[0, 0] = one                      # e_0
    qv[1, :] = mz                       # all -0.0: a zero norm
    qv[2, 0], qv[2, 1] = one, mz        # 1 x (-0.0 elsewhere)
    rv = np.zeros((4, 128), dtype=np.uint16)
    rv[0, 1] = neg                      # orthogonal to e_0, products 1 * 0 and 0 * (-1) = -0.0
    rv[1, :] = mz                       # a zero row of minus zeros
    rv[2, 0], rv[2, 1] = mz, neg        # dot with e_0: 1 * (-0.0) = -0.0, then + 0 * (-1) = -0.0
    rv[3, 1] = one
    for dtype in ("f16",):
        e = cref.cosine_matrix(qv, rv, dtype=dtype)
        assert (e == 0.0).all() and not np.signbit(e).any(), e
        seen_zero = True
    assert seen_zero
    # (2)
    e = np.concatenate(values + [np.array([0.0, 1.0, -1.0, 5e-324, -5e-324, 2.0 ** -1074, 1e308, -1e308])])
    assert not np.signbit(e[e == 0.0]).any()
    for z in (0.0, -0.0):
        assert np.array_equal(_bits64(e + np.float64(z)), _bits64(e))
        assert np.array_equal(_bits64(BR.bias_scores_loop(e, 1.0, np.full(e.size, z, np.float32))), _bits64(e))
    for beta in (1.0, -1.0, 0.3, -2.0 ** 20, 2.0 ** -20):
        assert beta * 0.0 == 0.0 and (-beta) * 0.0 == 0.0           # +-0.0, never anything else
    assert np.array_equal(_bits64(BR.bias_scores_loop(e, -0.5, np.zeros(e.size, np.float32))), _bits64(e))   # -0.5 * 0.0 = -0.0


# ---- the bound ------------------------------------------------------------------------------------------------------------
def test_eps_bias_restated_and_monotone():
    for D in (128, 384, 768, 2048):
        for B in (0.0, 1.0, -2.5, 2.0 ** -20, 1000.25, -2.0 ** 60):
            assert BR.eps_bias(D, B) == 2.0 * (D + 8) * 2.0 ** -24 + 2.0 ** -21 + 2.0 ** -22 * abs(B)
    assert BR.eps_bias(768, 0.0) == MR.cert_eps(768) + 2.0 ** -21
    assert BR.slack_m(1) == 9 and BR.slack_m(5) == 13 and BR.slack_m(64) == 80
    for beta in BR.BETAS:                                           # every scan weight is inside the domain, or zero
        assert beta == 0.0 or BR.W_MIN <= abs(beta) <= BR.W_MAX
    for name in BR.SETS:
        assert all(abs(BR.set_value(name, r, 17, 40)) <= BR.B_MAX for r in range(17, 57))
    # B + eps_bias(D, B) is increasing in B (slope 1 +- 2^-22): over fp32 values of both signs, neighbours included
    rng = np.random.default_rng(3)
    pats = rng.integers(0, 2 ** 32, size=200_000, dtype=np.uint64).astype(np.uint32)
    near = np.arange(-2000, 2000, dtype=np.int64)
    for centre in (0x00000000, 0x80000000, 0x3F800000, 0xBF800000, 0x447A0000, 0xC0400000, 0x7F000000, 0xFF000000):
        pats = np.concatenate([pats, ((centre + near) % 2 ** 32).astype(np.uint32)])
    B = pats.view(np.float32)
    B = np.unique(B[np.isfinite(B)]).astype(np.float64)             # ascending; -0.0 == +0.0 collapse
    assert B[0] < -1e37 and B[-1] > 1e37 and B.size > 150_000
    for D in (128, 2048):
        f = B + (MR.cert_eps(D) + 2.0 ** -21 + 2.0 ** -22 * np.abs(B))
        # as fp64 evaluates it, it never decreases (fp32 neighbours below 2^-50 or so collapse into one fp64 sum: the
        # certificate needs B_r <= B* => f(B_r) <= f(B*), which a weakly increasing f gives) ...
        assert (np.diff(f) >= 0).all()
        assert (np.diff(f)[np.abs(B[1:]) > 2.0 ** -20] > 0).all()
        # ... and in exact arithmetic it increases strictly, fp32 neighbours around zero included
        c = Fraction(MR.cert_eps(D)) + Fraction(2) ** -21
        z = int(np.searchsorted(B, 0.0))
        assert B[z] == 0.0 and B[z - 1] == -2.0 ** -149 and B[z + 1] == 2.0 ** -149
        for lo, hi in ((0, 3000), (z - 3000, z + 3000), (B.size - 3000, B.size)):
            exact = [Fraction(b) + c + Fraction(2) ** -22 * abs(Fraction(b)) for b in B[lo:hi]]
            assert all(x < y for x, y in zip(exact, exact[1:]))


@pytest.mark.parametrize("D,dtype", BR.DTS)
def test_the_bound_holds_for_the_epilogues_fp32_steps(D, dtype):
    """B as the scan's epilogue computes it, restated in numpy fp32 on an idealised scanned score s = fl32(e ||q||) (one
    rounding away from e ||q||; the scan's own error against e is cert_eps's part of the bound): coef = fl32(1 / ||q||),
    g = fl32(beta), B = fl32(fl32(coef * s) + fl32(g * b)).  |B - S| stays inside the rounding part of eps_bias,
    2^-21 + 2^-22 |B|: seven roundings of at most 2^-24 relative, on magnitudes bounded by 1 + |beta b| <= 2 + |B|."""
    worst = 0.0
    for shape in MR.SHAPES:
        rows, q, base, live = MR.host_dataset(D, dtype, shape)
        total, cap = MR.SHAPES[shape]
        n = live.shape[1]
        cols = BR.set_columns(base, n, cap or total)
        qn = np.linalg.norm(q.double().numpy(), axis=1)
        extra = ((0, 2.0 ** 20), (4, -2.0 ** 20), (3, 2.0 ** -20), (4, 1.0 / 3))
        for si, beta in [(si, beta) for si in range(5) for beta in BR.BETAS] + list(extra):
            b = BR.row_bias(cols[si:si + 1], None, 1, base, n, cap or total)[0]
            for qi in range(BR.NQ):
                S = BR.bias_scores_loop(live[qi], beta, b)
                s = (live[qi] * qn[qi]).astype(np.float32)
                coef, g = np.float32(1.0 / qn[qi]), np.float32(beta)
                B = ((coef * s).astype(np.float32) + (g * b).astype(np.float32)).astype(np.float32).astype(np.float64)
                room = 2.0 ** -21 + 2.0 ** -22 * np.abs(B)
                assert (np.abs(B - S) <= room).all(), (shape, si, beta, qi)
                assert (np.abs(B - S) <= [BR.eps_bias(D, x) for x in B]).all()
                worst = max(worst, float((np.abs(B - S) / room).max()))
    print(f"D={D} {dtype}: worst |B - S| = {worst:.3f} of the rounding part of eps_bias")
    assert 0.0 < worst <= 1.0


# ---- the Python layer, before the library is called ---------------------------------------------------------------------
def test_python_refusals_and_scratch():
    from tests.host_memory import host_memory
    from tests.host_memory import SizingLibrary
    from vidmem import memory as M
    mem = host_memory(capacity=100)
    S = mem.bias_stride
    assert S == 128 == BR.bias_stride(100) == 32 * mem.mask_words
    q = torch.zeros((3, mem.dim))
    col = mem.new_bias()
    assert col.shape == (1, S) and col.dtype == torch.float32 and not col.any()
    assert mem.new_bias(4).shape == (4, S)
    for k in (0, 65):
        with pytest.raises(ValueError, match="k"):
            mem.topk_biased(q, k, col)
    with pytest.raises(ValueError, match="float32"):
        mem.topk_biased(q, 3, col.double())
    with pytest.raises(ValueError, match="float32"):
        mem.topk_biased(q, 3, [0.0] * S)
    with pytest.raises(ValueError, match="width"):
        mem.topk_biased(q, 3, torch.zeros(S + 64))
    with pytest.raises(ValueError, match="n_bias"):
        mem.topk_biased(q, 3, torch.zeros((0, S)))
    with pytest.raises(ValueError, match="is on"):
        mem.topk_biased(q, 3, torch.zeros(S, device="meta"))
    with pytest.raises(ValueError, match="bias_index"):
        mem.topk_biased(q, 3, mem.new_bias(2))
    with pytest.raises(ValueError, match="bias indices"):
        mem.topk_biased(q, 3, mem.new_bias(2), bias_index=[0, 1])
    with pytest.raises(ValueError, match="int32"):
        mem.topk_biased(q, 3, mem.new_bias(2), bias_index=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="weights for"):
        mem.topk_biased(q, 3, col, weight=[1.0, 2.0])
    with pytest.raises(ValueError, match="float64"):
        mem.topk_biased(q, 3, col, weight=torch.ones(3))
    with pytest.raises(ValueError, match="dimension"):
        mem.topk_biased(torch.zeros((3, mem.dim + 1)), 3, col)
    with pytest.raises(ValueError, match="width"):
        mem.topk_biased(q, 3, col, mask=torch.zeros(mem.mask_words + 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="mask_index"):
        mem.topk_biased(q, 3, col, mask=torch.zeros((2, mem.mask_words), dtype=torch.int32))
    with pytest.raises(ValueError, match="needs a mask"):
        mem.topk_biased(q, 3, col, mask_index=[0, 0, 0])
    with pytest.raises(ValueError, match="NaN"):
        mem.topk_biased(q, 3, col, min_score=float("nan"))
    with pytest.raises(ValueError, match="tagged"):
        mem.bias_of_age(0, 1e-6)
    with pytest.raises(ValueError, match="int64"):
        mem.bias_of_rows(torch.zeros(3, dtype=torch.int32), [1.0] * 3)
    with pytest.raises(ValueError, match="float32"):
        mem.bias_of_rows([1, 2, 3], torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="values for"):
        mem.bias_of_rows([1, 2, 3], [1.0, 2.0])
    with pytest.raises(ValueError, match="out must be"):
        mem.bias_of_rows([1], [1.0], out=torch.zeros(S + 1))
    with pytest.raises(ValueError, match="out must be"):
        host_memory(tagged=True, capacity=100).bias_of_age(0, 1e-6, out=mem.new_bias(2))
    sized = host_memory(capacity=16, library=SizingLibrary())
    first = sized.prepare_topk_biased(4, 10)                        # the stand-in sizes any vm_*_workspace_bytes entry
    assert isinstance(first, M.BiasTopkScratch) and first.fits(sized, 4, 10)
    assert first.ws.numel() == 1000 + 64 * 14 and first.flags.dtype == torch.int32
    assert sized.prepare_topk_biased(2, 5) is first                 # a smaller call uses the same scratch
    assert sized.prepare_topk_biased(64, 32) is not first           # one that does not fit is replaced, never resized
    other = M.BiasTopkScratch.for_(sized, 2, 2)
    with pytest.raises(ValueError, match="too small"):
        sized._resolve(M.BiasTopkScratch, other, 64, 32)            # a caller-owned scratch must fit
    assert mem.last_bias_flags is None and mem.bias_uncertified_count == 0


def test_header_and_library():
    from vidmem import _lib
    text = open(os.path.join(ROOT, "include", "vidmem.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("S(q, r) = e(q, r) + beta_q * b[slot(r)]",
                   "one fp64 rounding for the product and one for the sum, never fused",
                   "An index outside [0, n_bias) is the ZERO column",
                   "S > min_score",
                   "eps_bias(D, B) = 2 (D + 8) 2^-24 + 2^-21 + 2^-22 |B|",
                   "|beta| is 0 or lies in [2^-20, 2^20]",
                   "|b| <= 2^40",
                   "the reference cosine is never -0.0",
                   "Duplicates that carry DIFFERENT values leave one of them",
                   "More than 2^30 bias values",
                   "not on the other queries of the call"):
        assert phrase in flat, phrase
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for decl in (r"int64_t vm_memory_bias_stride\(const vm_memory \*mem\);",
                 r"size_t vm_topk_bias_workspace_bytes\(const vm_memory \*mem, int Q, int k\);",
                 r"int vm_topk_cosine_biased\(vm_memory \*mem, const void \*queries, int Q, int k, const float \*bias, "
                 r"int n_bias,",
                 r"int vm_topk_cosine_biased_exact\(vm_memory \*mem, const void \*queries, int Q, int k, const float \*bias, "
                 r"int n_bias,",
                 r"int vm_bias_from_rows\(vm_memory \*mem, const int64_t \*row_ids, const float \*values, int64_t n,",
                 r"int vm_bias_from_tags\(vm_memory \*mem, int64_t t_ref_ms, double per_ms, float fill, float \*out_bias,"):
        assert re.search(decl, code), decl
    L = _lib.lib()
    assert L.vm_abi_version() == 4
    for sym in ("vm_memory_bias_stride", "vm_topk_bias_workspace_bytes", "vm_topk_cosine_biased",
                "vm_topk_cosine_biased_exact", "vm_bias_from_rows", "vm_bias_from_tags"):
        assert sym in _lib.SYMBOLS
        getattr(L, sym)
    assert L.vm_memory_bias_stride(None) == 0
    assert L.vm_topk_bias_workspace_bytes(None, 1, 1) == 0
    assert L.vm_topk_cosine_biased(None, None, 1, 1, None, 1, None, None, None, 0, None, 0, 0.0, 1, 0, None, None, None,
                                   None, None, 0, None) == _lib.VM_ERR_INVALID
    assert L.vm_topk_cosine_biased_exact(None, None, 1, 1, None, 1, None, None, None, 0, None, 0, 0.0, 1, 0, None, None,
                                         None, 0, None) == _lib.VM_ERR_INVALID
    assert L.vm_bias_from_rows(None, None, None, 0, 1, 0, 1, None, None) == _lib.VM_ERR_INVALID
    assert L.vm_bias_from_tags(None, 0, 1e-6, 0.0, None, None) == _lib.VM_ERR_INVALID


# ---- planted defects: statement (A) tells each of them from the contract on the scan test's own data --------------------
def _scan_case(shape="ring40", D=128, dtype="f16"):
    rows, q, base, live, cap = _case(D, dtype, shape)
    n = live.shape[1]
    cols = BR.set_columns(base, n, cap, dead=0.0)
    index = [BR.query_case(i)[0] for i in range(33)]
    betas = [BR.query_case(i)[1] for i in range(33)]
    return live, base, n, cap, cols, index, betas


def _differs(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(_bits64(a[1]), _bits64(b[1])))


def test_planted_bias_indexed_by_row_id_instead_of_slot():
    live, base, n, cap, cols, index, betas = _scan_case("ring40")
    assert base == 17 and cap == 40 and cols.shape[1] == 64         # row ids 17 .. 56 fit a column, slots wrap
    good = BR.row_bias(cols, index, 33, base, n, cap)
    by_id = np.stack([cols[index[qi]][base + np.arange(n)] for qi in range(33)])     # the defect: b[r], not b[r % cap]
    want = BR.bias_topk_from_cosines(live, betas, good, None, 5, base=base)
    bad = BR.bias_topk_from_cosines(live, betas, by_id, None, 5, base=base)
    assert _differs(want, bad)
    seen = [qi for qi in range(33) if _differs((want[0][qi], want[1][qi]), (bad[0][qi], bad[1][qi]))]
    assert all(index[qi] != 0 and betas[qi] != 0.0 for qi in seen)  # only where a set and a weight are live ...
    assert len(seen) >= 8, seen                                     # ... and a row id >= 40 reaches the top 5


def test_planted_weight_applied_to_the_cosine():
    live, base, n, cap, cols, index, betas = _scan_case("n47")
    b = BR.row_bias(cols, index, 33, base, n, cap)
    want = BR.bias_topk_from_cosines(live, betas, b, None, 5, base=base)
    bad = BR.bias_topk_from_cosines(live, betas, b, None, 5, base=base,
                                    scores=lambda e, beta, bb: np.array([float(beta) * float(x) + float(y)
                                                                         for x, y in zip(e, bb)]))
    for qi in range(33):
        if betas[qi] != 1.0:
            assert _differs((want[0][qi], want[1][qi]), (bad[0][qi], bad[1][qi])), qi


def test_planted_sum_taken_in_fp32():
    live, base, n, cap, cols, index, betas = _scan_case("n33")
    b = BR.row_bias(cols, index, 33, base, n, cap)
    want = BR.bias_topk_from_cosines(live, betas, b, None, 5, base=base)
    bad = BR.bias_topk_from_cosines(live, betas, b, None, 5, base=base,
                                    scores=lambda e, beta, bb: np.array(
                                        [float(np.float32(float(x) + float(beta) * float(y))) for x, y in zip(e, bb)]))
    assert sum(_differs((want[0][qi], want[1][qi]), (bad[0][qi], bad[1][qi])) for qi in range(33)) >= 30


def _fma(a: float, b: float, c: float) -> float:
    """a * b + c with ONE rounding: exact rational arithmetic, then the correctly rounded quotient of two integers."""
    x = Fraction(a) * Fraction(b) + Fraction(c)
    return x.numerator / x.denominator


def test_planted_fma_in_place_of_the_two_roundings():
    """A kernel that contracts ``e + beta * b`` into one fused multiply-add rounds once.  The GPU test can see that only if
    some (query, row) of the scan data scores other bits under an FMA - shown here for every shape, and for the results."""
    assert _fma(0.1, 3.0, -0.3) != 0.1 * 3.0 + -0.3                 # the restatement does fuse
    pairs = 0
    for shape in MR.SHAPES:
        live, base, n, cap, cols, index, betas = _scan_case(shape)
        b = BR.row_bias(cols, index, 33, base, n, cap)
        fused = lambda e, beta, bb: np.array([_fma(float(beta), float(y), float(x)) for x, y in zip(e, bb)])
        here = 0
        for qi in range(33):
            two = BR.bias_scores_loop(live[qi], betas[qi], b[qi])
            here += int((_bits64(two) != _bits64(fused(live[qi], betas[qi], b[qi]))).sum())
        assert here >= 1, shape
        pairs += here
        want = BR.bias_topk_from_cosines(live, betas, b, None, 5, base=base)
        bad = BR.bias_topk_from_cosines(live, betas, b, None, 5, base=base, scores=fused)
        assert _differs(want, bad), shape                           # and it reaches the top 5 of some query
    print(f"{pairs} (query, row) pairs of the scan data differ under an FMA")


def test_planted_out_of_range_index_not_the_zero_column():
    live, base, n, cap, cols, index, betas = _scan_case("n47")
    index = [7, -1, 5] + index[3:]
    betas = [1.0, 0.3, -0.5] + betas[3:]
    want = BR.bias_topk_from_cosines(live, betas, BR.row_bias(cols, index, 33, base, n, cap), None, 5, base=base)
    clamped = [min(max(i, 0), 4) for i in index]                    # the defect: the index clamped into range
    bad = BR.bias_topk_from_cosines(live, betas, BR.row_bias(cols, clamped, 33, base, n, cap), None, 5, base=base)
    plain = MR.masked_topk_from_scores(live, np.ones_like(live, dtype=bool), 5, base=base)
    for qi in (0, 2):                                               # clamped to 'big', against the plain cosine order
        assert _differs((want[0][qi], want[1][qi]), (bad[0][qi], bad[1][qi])), qi
    for qi in range(3):
        assert not _differs((want[0][qi], want[1][qi]), (plain[0][qi], plain[1][qi])), qi


# ---- the GPU scan test's precondition ------------------------------------------------------------------------------------
def test_scan_precondition_every_set_and_weight_unmasked():
    """For the five sets and the five weights, every shape, D and dtype, all 33 queries and k in (1, 5), without a mask:
    rank k and rank M + 1 of the oracle's S are more than 4 x eps_bias apart, so the fast path must certify."""
    cases = 0
    smallest = (np.inf, None)
    for D, dtype in BR.DTS:
        for shape in MR.SHAPES:
            S = BR.scan_scores(D, dtype, shape)
            for (si, beta), mat in S.items():
                for qi in range(BR.NQ):
                    best = np.sort(mat[qi])[::-1]
                    for k in BR.KS:
                        m = BR.margin(best, k, D)
                        cases += 1
                        assert BR.flag0_ok(best, k, D), (D, dtype, shape, BR.SETS[si], beta, qi, k, m)
                        if m < smallest[0]:
                            smallest = (m, (D, dtype, shape, BR.SETS[si], beta, qi, k))
    print(f"{cases} unmasked cases hold; smallest margin {smallest[0]:.1f} x eps_bias at {smallest[1]}")
    assert cases == 26_400 and smallest[0] > 4


def test_scan_precondition_of_the_gpu_tests_own_cases():
    """The GPU scan test's cases exactly - query i takes set (i // 5) % 5 and weight BETAS[i % 5], Q in (1, 17, 33), no
    mask and every mask set - keep the flag-0 demand for at least 0.9 of the cases of EVERY (shape, D, dtype), which is
    what each parametrised GPU case asserts."""
    kept_all = total_all = 0
    for D, dtype in BR.DTS:
        for shape in MR.SHAPES:
            _, _, base, live = MR.host_dataset(D, dtype, shape)
            n = live.shape[1]
            S = BR.scan_scores(D, dtype, shape)
            kept = total = 0
            for Q in BR.QS:
                for name, sel in BR.scan_selections(Q, shape, base, n).items():
                    for qi in range(Q):
                        si, beta = BR.query_case(qi)
                        best = np.sort(S[si, beta][qi][sel[qi]])[::-1]
                        for k in BR.KS:
                            ok = BR.flag0_ok(best, k, D)
                            assert ok or name != "none"
                            total += 1
                            kept += ok
            assert kept >= 0.9 * total, (D, dtype, shape, kept, total)
            kept_all += kept
            total_all += total
    print(f"{kept_all} of {total_all} cases of the GPU scan test keep the flag-0 demand")
