"""GPU: each encoder GEMM kernel and epilogue alone, element by element against fp64 (tests/stage_ref.py).

Every case builds its 16-bit operands from seeded generators, launches vm_gemm through the test shim
(tests/stage_lib.py: the release library's own object code), and compares EVERY output element with the fp64
restatement under the derived element-wise bound - no norm, no excluded element.  The fp64 reference is computed on the
device (rocBLAS dgemm shares nothing with the kernels under test); the small grid also runs it on the CPU once to show
the two agree.  Outputs are windows inside larger canary-filled allocations (>= 512 guard rows before, behind and
between head blocks): the guards and every row the launcher's contract leaves alone must still hold the canary.
Which kernel a case takes is asserted with the dispatch mirror for the device's CU count, never assumed.
"""
import time

import pytest
import torch

import tests.stage_cases as CS
import tests.stage_ref as R
from tests.stage_lib import Stages

pytestmark = pytest.mark.gpu

DTYPES = ("f16", "bf16")
G = CS.GUARD_ROWS
DEV = "cuda"


@pytest.fixture(scope="module")
def st():
    t0 = time.time()
    s = Stages(0)
    yield s
    s.set_variant(0)
    CS.flush_record("gemm", time.time() - t0)


def run16(st, dtype, epi, X, W, bias, M, N, K, *, ldx=None, row_step=1, row_len=None, total_rows=None,
          head_major=False, hm_stride=1, n_off_blocks=0, heads_total=None):
    """Launch one 16-bit-output GEMM into a canary-filled window; return the [M, N] outputs (fp32 view of the stored
    values) after asserting that nothing else was written.

    row-major: the window is [total_rows, row_len] (GEMM row t at window row t * row_step, ldo = row_step * row_len).
    head-major: [blocks][hm_rows][64] with hm_rows = M * hm_stride + 512 (so 512 canary rows part the head blocks), the
    GEMM writing blocks n_off_blocks .. n_off_blocks + N/64 of heads_total."""
    kind = R.out_kind(dtype, epi)
    if head_major:
        hm_rows = M * hm_stride + G
        blocks = heads_total or N // 64
        buf = CS.canary16(G + blocks * hm_rows + G, 64, DEV)
        win = buf[G:G + blocks * hm_rows].view(blocks, hm_rows, 64)
        out_ptr = win[n_off_blocks]
        st.gemm(dtype, epi, X, W, bias, out16=out_ptr, M=M, N=N, K=K, ldx=ldx, ldo=N, head_major=1, hm_rows=hm_rows,
                hm_stride=hm_stride)
        torch.cuda.synchronize()
        sel = win[n_off_blocks:n_off_blocks + N // 64, 0:M * hm_stride:hm_stride, :]     # [N/64, M, 64]
        got = sel.permute(1, 0, 2).reshape(M, N).clone()
        sel.fill_(CS.CANARY16)
    else:
        row_len = row_len or N
        total_rows = total_rows or M
        buf = CS.canary16(G + total_rows + G, row_len, DEV)
        win = buf[G:G + total_rows]
        st.gemm(dtype, epi, X, W, bias, out16=win, M=M, N=N, K=K, ldx=ldx, ldo=row_step * row_len)
        torch.cuda.synchronize()
        sel = win[0:M * row_step:row_step, :N]
        got = sel.clone()
        sel.fill_(CS.CANARY16)
    assert CS.untouched(buf), "a 16-bit GEMM epilogue wrote outside its [M, N] outputs"
    return got.view(R.TDT[kind]).float()


def run32(st, dtype, epi, X, W, bias, M, N, K, *, resid=None, pos=None, P=0, T=0):
    """EPI_RESID32 (in place on `resid` [M, N]) or EPI_PATCH (row frame*T + 1 + p of a [frames*T, N] window)."""
    if epi == R.EPI_RESID32:
        rows = M
        buf = CS.canary32(G + rows + G, N, DEV)
        win = buf[G:G + rows]
        win.view(torch.float32).copy_(resid)
        st.gemm(dtype, epi, X, W, bias, out32=win, M=M, N=N, K=K)
        torch.cuda.synchronize()
        got = win.view(torch.float32).clone()
        win.fill_(CS.CANARY32)
    else:
        frames = M // P
        assert frames * P == M
        buf = CS.canary32(G + frames * T + G, N, DEV)
        win = buf[G:G + frames * T].view(frames, T, N)
        st.gemm(dtype, epi, X, W, bias, out32=win, pos=pos, M=M, N=N, K=K, P=P, T=T)
        torch.cuda.synchronize()
        got = win[:, 1:1 + P, :].reshape(M, N).view(torch.float32).clone()
        win[:, 1:1 + P, :].fill_(CS.CANARY32)     # row frame * T (the CLS row) and rows past 1 + P stay canary
    assert CS.untouched(buf), "an fp32 GEMM epilogue wrote outside its rows"
    return got


def check(family_case, got, y, bound):
    ratio, outside = R.worst_ratio(got, y, bound)
    print(f"{family_case}: worst error / bound = {ratio:.4f}, outside = {outside} of {y.numel()}")
    CS.record("gemm", family_case, ratio)
    assert outside == 0, f"{family_case}: {outside} of {y.numel()} elements outside the bound (worst ratio {ratio:.3f})"


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm128_shape_grid(st, dtype):
    """gemm128_kernel at its own edges (stage_cases.gemm_grid_shapes), EPI_STORE16.  The fp64 reference of every shape is
    also computed on the CPU: device dgemm and CPU must agree to the fp64 rounding of two K-term sums."""
    full = CS.gemm_inputs(11, "grid." + dtype, dtype, 197 * 3, 768, 768, DEV)
    for M, N, K in CS.gemm_grid_shapes():
        assert R.gemm_plan(M, N, K, st.num_cus)["kernel"] == "gemm128"
        X = full["X"][:M, :K].contiguous()
        W = full["W"][:N, :K].contiguous()
        b = full["bias"][:N].contiguous()
        got = run16(st, dtype, R.EPI_STORE16, X, W, b, M, N, K)
        y, bound = R.gemm_ref_and_bound(dtype, R.EPI_STORE16, X, W, b, K)
        y_cpu, _ = R.gemm_ref_and_bound(dtype, R.EPI_STORE16, X.cpu(), W.cpu(), b.cpu(), K)
        _, A = R.gemm_pre(X, W, b)
        # two fp64 sums of K products and a bias in different orders: each within (K + 1) 2^-53 A of the exact value
        assert bool(((y.cpu() - y_cpu).abs() <= 2.0 * (K + 1) * 2.0 ** -53 * A.cpu()).all()), \
            "device and CPU fp64 references disagree"
        check(f"{dtype}.grid.M{M}.N{N}.K{K}", got, y, bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("idx", range(4))
def test_gemm_named_paths(st, dtype, idx):
    """The persistent kernel under automatic dispatch (ragged last panel; several tiles per workgroup with non-temporal
    stores; feature-group tile order) and gemm256_kernel under automatic dispatch (N > 4096)."""
    case = CS.gemm_cases(st.num_cus)[idx]
    M, N, K = case["M"], case["N"], case["K"]
    plan = R.gemm_plan(M, N, K, st.num_cus)
    for key, want in case["expect"].items():
        assert plan[key] == want, f"{case['name']}: dispatch mirror says {key} = {plan[key]} for {st.num_cus} CUs"
    assert plan["tiles_per_wg"] >= case.get("min_tiles_per_wg", 1)
    ins = CS.gemm_inputs(12 + idx, case["name"] + dtype, dtype, M, N, K, DEV)
    st.ctx.profile_enable(16)
    st.ctx.profile_read()
    got = run16(st, dtype, R.EPI_STORE16, ins["X"], ins["W"], ins["bias"], M, N, K)
    launches = st.ctx.profile_read()
    st.ctx.profile_enable(0)
    assert launches["gemm_qkv"][1] == 1, "vm_gemm did not launch exactly one kernel in the category it was given"
    y, bound = R.gemm_ref_and_bound(dtype, R.EPI_STORE16, ins["X"], ins["W"], ins["bias"], K)
    check(f"{dtype}.{case['name']}", got, y, bound)


EPIS16 = (R.EPI_STORE16, R.EPI_DELTA16, R.EPI_GELU16, R.EPI_QGELU16)
EPI_NAME = {0: "STORE16", 1: "GELU16", 2: "QGELU16", 3: "RESID32", 4: "PATCH", 5: "DELTA16"}


def epi_shape(st, which):
    """128^2 kernel: three ragged 128-row tiles; persistent kernel: its automatic shape with the ragged last panel.
    K = 64 keeps the accumulation term negligible: the activations are judged at u_out plus their approximation error."""
    if which == "gemm128":
        return 197 * 3, 256, 64
    c = CS.gemm_cases(st.num_cus)[0]
    return c["M"], c["N"], c["K"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ("gemm128", "gemm256p"))
@pytest.mark.parametrize("epi", (0, 5, 1, 2, 3))
def test_gemm_epilogues(st, dtype, which, epi):
    """STORE16, DELTA16, GELU16, QGELU16 and RESID32 on the 128^2 and on the persistent kernel (PATCH: its own test
    below).  Pre-activations of spread 2.5: the GELU inputs cover +-6 and beyond."""
    M, N, K = epi_shape(st, which)
    assert R.gemm_plan(M, N, K, st.num_cus)["kernel"] == which
    ins = CS.gemm_inputs(20, f"epi.{which}.{dtype}", dtype, M, N, K, DEV, z_std=2.5)
    if epi == R.EPI_RESID32:
        resid = CS.t32(CS.syn.normal(21, "epi.resid", (M, N), std=4.0), DEV)
        got = run32(st, dtype, epi, ins["X"], ins["W"], ins["bias"], M, N, K, resid=resid)
        y, bound = R.gemm_ref_and_bound(dtype, epi, ins["X"], ins["W"], ins["bias"], K, extra=resid)
    else:
        got = run16(st, dtype, epi, ins["X"], ins["W"], ins["bias"], M, N, K)
        y, bound = R.gemm_ref_and_bound(dtype, epi, ins["X"], ins["W"], ins["bias"], K)
    check(f"{dtype}.{which}.{EPI_NAME[epi]}", got, y, bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ("gemm128", "gemm256p"))
@pytest.mark.parametrize("P", (196, 576))
def test_gemm_patch_rows(st, dtype, which, P):
    """EPI_PATCH: GEMM row frame * P + p lands in token row frame * T + 1 + p (T = P + 1) with pos[1 + p] added; row
    frame * T (the CLS row) is untouched.  Frames: 3 on the 128^2 kernel, enough for the persistent one otherwise."""
    T, N, K = P + 1, 256, 64
    frames = 3 if which == "gemm128" else -(-(256 * -(-8 * st.num_cus // 10)) // P) + 1
    M = frames * P
    assert R.gemm_plan(M, N, K, st.num_cus)["kernel"] == which
    ins = CS.gemm_inputs(30, f"patch.{which}.{dtype}.{P}", dtype, M, N, K, DEV)
    pos = CS.t32(CS.syn.normal(31, f"patch.pos.{P}", (T, N), std=1.0), DEV)
    got = run32(st, dtype, R.EPI_PATCH, ins["X"], ins["W"], ins["bias"], M, N, K, pos=pos, P=P, T=T)
    extra = pos[1:1 + P].repeat(frames, 1)
    y, bound = R.gemm_ref_and_bound(dtype, R.EPI_PATCH, ins["X"], ins["W"], ins["bias"], K, extra=extra)
    check(f"{dtype}.{which}.PATCH.P{P}", got, y, bound)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_variants_agree_bit_for_bit(st, dtype):
    """gemm.hip: all tilings accumulate each output in the same MFMA order - so the three kernels, forced through
    vm_gemm_set_variant(1 / 2 / 3), must agree bit for bit for every 16-bit epilogue (and each lies inside the bound)."""
    M, N, K = 300, 512, 128
    ins = CS.gemm_inputs(40, "variants." + dtype, dtype, M, N, K, DEV, z_std=2.5)
    try:
        for epi in EPIS16:
            y, bound = R.gemm_ref_and_bound(dtype, epi, ins["X"], ins["W"], ins["bias"], K)
            outs = {}
            for variant, kernel in ((1, "gemm128"), (2, "gemm256"), (3, "gemm256p")):
                assert R.gemm_plan(M, N, K, st.num_cus, variant=variant)["kernel"] == kernel
                st.set_variant(variant)
                outs[variant] = run16(st, dtype, epi, ins["X"], ins["W"], ins["bias"], M, N, K)
                check(f"{dtype}.variant{variant}.{EPI_NAME[epi]}", outs[variant], y, bound)
            assert torch.equal(outs[1], outs[2]) and torch.equal(outs[1], outs[3]), \
                f"{EPI_NAME[epi]}: the three GEMM kernels do not agree bit for bit"
    finally:
        st.set_variant(0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("epi", (R.EPI_GELU16, R.EPI_QGELU16))
def test_gemm_activation_dense_sweep(st, dtype, epi):
    """The pre-activation takes every value of the 16-bit type in [-6, 6] once and is exact in the kernel (K = 64, one
    non-zero product per sum): the activations are held to u_out plus their documented approximation error alone."""
    ins = CS.gelu_sweep_inputs(dtype, DEV)
    M, N, K = ins["M"], ins["N"], ins["K"]
    got = run16(st, dtype, epi, ins["X"], ins["W"], ins["bias"], M, N, K)
    y, bound = R.gemm_ref_and_bound(dtype, epi, ins["X"], ins["W"], ins["bias"], K, exact_pre=True)
    z, _ = R.gemm_pre(ins["X"], ins["W"], ins["bias"])
    want = torch.cat([CS.sweep_values(dtype).double(), -CS.sweep_values(dtype).double()]).unique()
    assert torch.equal(z.cpu().flatten().unique(), want), "the sweep does not cover every value in [-6, 6]"
    check(f"{dtype}.sweep.{EPI_NAME[epi]}", got, y, bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ("gemm128", "gemm256p"))
def test_gemm_delta16_range(st, dtype, which):
    """EPI_DELTA16 beyond fp16's range.  CONTRACT (csrc/vm_kernels.h, gemm.hip sat_f16): a bf16 encoder's branch output
    saturates at +-65504 and a NaN stays a NaN; for an fp16 encoder EPI_DELTA16 IS EPI_STORE16 ("Same as STORE16 for
    fp16": one instantiation), so a sum beyond the range overflows to +-inf as IEEE rounding says, and a NaN stays a NaN.
    Bias columns 0 / 1 / 2 carry +1e5 / -1e5 / NaN; every other column is checked under the ordinary bound."""
    M, N, K = (130, 256, 64) if which == "gemm128" else epi_shape(st, which)
    assert R.gemm_plan(M, N, K, st.num_cus)["kernel"] == which
    ins = CS.gemm_inputs(50, f"sat.{which}.{dtype}", dtype, M, N, K, DEV)
    bias = ins["bias"].clone()
    bias[0], bias[1], bias[2] = 1e5, -1e5, float("nan")
    got = run16(st, dtype, R.EPI_DELTA16, ins["X"], ins["W"], bias, M, N, K)
    big = R.F16_MAX if dtype == "bf16" else float("inf")
    assert bool((got[:, 0] == big).all()) and bool((got[:, 1] == -big).all()), f"beyond-range columns are not +-{big}"
    assert bool(torch.isnan(got[:, 2]).all()), "a NaN pre-activation did not stay a NaN"
    y, bound = R.gemm_ref_and_bound(dtype, R.EPI_DELTA16, ins["X"], ins["W"], ins["bias"], K)
    check(f"{dtype}.{which}.DELTA16.range", got[:, 3:], y[:, 3:], bound[:, 3:])


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_addressing_as_attn_block_uses_it(st, dtype):
    """The three addressings of the last layer's CLS-only path and of the split QKV call:
      (a) head_major with hm_rows / hm_stride: a GEMM over the B CLS rows (ldx = T * H) writing row b * T of each q block;
      (b) ldx = T * H and ldo = T * H: the CLS-rows-only projection (row-major, rows b * T of a [B * T, H] array), and
          FC1 + activation / FC2 the same way with N != K (ldx = T * K, ldo = T * N);
      (c) the K/V-only QKV call: W and bias offset by H rows, the output offset by `heads` blocks of a [3 * heads] array.
    Everything between the written rows must keep the canary."""
    B, T, H, heads = 37, 17, 256, 4
    K = H
    act = CS.gemm_inputs(60, "addr." + dtype, dtype, B * T, 3 * H, K, DEV)       # activations [B*T, H], W [3H, H]
    Xall, Wqkv, bqkv = act["X"], act["W"], act["bias"]
    Xcls = Xall[::T]
    # (a) q of the CLS rows, head-major, block row b * T
    hm_rows = B * T + G
    buf = CS.canary16(G + heads * hm_rows + G, 64, DEV)
    win = buf[G:G + heads * hm_rows].view(heads, hm_rows, 64)
    st.gemm(dtype, R.EPI_STORE16, Xall, Wqkv, bqkv, out16=win, M=B, N=H, K=K, ldx=T * H, ldo=H, head_major=1,
            hm_rows=hm_rows, hm_stride=T)
    torch.cuda.synchronize()
    sel = win[:, 0:B * T:T, :]
    got = sel.permute(1, 0, 2).reshape(B, H).clone().view(R.TDT[dtype]).float()
    sel.fill_(CS.CANARY16)
    assert CS.untouched(buf), "the CLS-query GEMM wrote outside rows b * T of its head blocks"
    y, bound = R.gemm_ref_and_bound(dtype, R.EPI_STORE16, Xcls, Wqkv[:H], bqkv[:H], K)
    check(f"{dtype}.addr.cls_query_head_major", got, y, bound)
    # (b) CLS rows only, row-major in and out, both strided by T * H; DELTA16 as the projection / FC2 store it
    got = run16(st, dtype, R.EPI_DELTA16, Xall, Wqkv[:H].contiguous(), bqkv[:H].contiguous(), B, H, K, ldx=T * H,
                row_step=T, row_len=H, total_rows=B * T)
    y, bound = R.gemm_ref_and_bound(dtype, R.EPI_DELTA16, Xcls, Wqkv[:H], bqkv[:H], K)
    check(f"{dtype}.addr.cls_rows_strided", got, y, bound)
    # (b') the same strided addressing through an MLP of the CLS rows with N != K: FC1 + activation (64 -> 256: K = 64
    # keeps the accumulation term below the activation's own error) and FC2 (256 -> 128, DELTA16 out), each reading
    # row b * T of its input and writing row b * T of its output
    Hs, Mlp, Ho = 64, 256, 128
    fc1 = CS.gemm_inputs(61, "addr.fc1." + dtype, dtype, B * T, Mlp, Hs, DEV, z_std=2.5)
    for epi in (R.EPI_GELU16, R.EPI_QGELU16):
        got = run16(st, dtype, epi, fc1["X"], fc1["W"], fc1["bias"], B, Mlp, Hs, ldx=T * Hs, row_step=T, row_len=Mlp,
                    total_rows=B * T)
        y, bound = R.gemm_ref_and_bound(dtype, epi, fc1["X"][::T], fc1["W"], fc1["bias"], Hs)
        check(f"{dtype}.addr.cls_rows_fc1.{EPI_NAME[epi]}", got, y, bound)
    fc2 = CS.gemm_inputs(62, "addr.fc2." + dtype, dtype, B * T, Ho, Mlp, DEV)
    got = run16(st, dtype, R.EPI_DELTA16, fc2["X"], fc2["W"], fc2["bias"], B, Ho, Mlp, ldx=T * Mlp, row_step=T, row_len=Ho,
                total_rows=B * T)
    y, bound = R.gemm_ref_and_bound(dtype, R.EPI_DELTA16, fc2["X"][::T], fc2["W"], fc2["bias"], Mlp)
    check(f"{dtype}.addr.cls_rows_fc2", got, y, bound)
    # (c) K and V of all rows: weights / bias from row H on, output blocks heads .. 3 * heads
    M = B * T
    got = run16(st, dtype, R.EPI_STORE16, Xall, Wqkv[H:], bqkv[H:], M, 2 * H, K, head_major=True, n_off_blocks=heads,
                heads_total=3 * heads)
    y, bound = R.gemm_ref_and_bound(dtype, R.EPI_STORE16, Xall, Wqkv[H:], bqkv[H:], K)
    check(f"{dtype}.addr.kv_only", got, y, bound)
