"""CPU: the bounds of tests/stage_ref.py are proven before they judge a kernel.

For every GPU case of tests/test_stage_*_gpu.py (the same case tables and seeded inputs of tests/stage_cases.py, at
reduced size: fewer token panels / sequences / rows, the same widths, tile edges and code paths) this file asserts:

  1. An INDEPENDENT emulation of the kernel's arithmetic - the same 16-bit inputs, torch fp32 accumulation in torch's own
     (different) order, the same rounding points taken with the rounders oracle/vit_ref.py uses (x.to(dtype).float()) -
     lies within the bound on 100 % of the elements.  Nothing is excluded; a NaN counts as outside.
  2. Each planted defect of the kernel family, applied to that emulation, puts at least one element outside.  A defect
     that cannot exist in a case is not planted there, and the rule is written where it is decided: a one-row GEMM or
     LayerNorm has no neighbouring row, T = 1 has no second key for a scale error to act on, a null deltaB16 cannot be
     folded twice, `eps omitted` needs the constant row that cases of three rows or more carry.

The reference itself is plain fp64 (stage_ref); the emulation shares no code with it beyond the input tensors.
"""
import itertools
import math

import pytest
import torch

import tests.stage_cases as CS
import tests.stage_ref as R

DTYPES = ("f16", "bf16")
CPU = "cpu"
EPI_NAME = {0: "STORE16", 1: "GELU16", 2: "QGELU16", 3: "RESID32", 4: "PATCH", 5: "DELTA16"}


def inside(got, y, bound, what):
    ratio, outside = R.worst_ratio(got, y, bound)
    assert outside == 0, f"{what}: the emulation leaves the bound on {outside} of {y.numel()} elements (ratio {ratio:.3f})"
    return ratio


def leaves(got, y, bound, what):
    _, outside = R.worst_ratio(got, y, bound)
    assert outside > 0, f"{what}: the planted defect stays inside the bound - inputs or bound too loose to be worth a GPU run"


# ======================================================================================================================
# GEMM
# ======================================================================================================================
TAB_A, TAB_B = R.gelu_table()


def emulate_gemm(dtype, epi, X, W, bias, K, extra=None, defect=None):
    """fp32 restatement with torch's own accumulation order; `defect` plants one of the listed kernel errors."""
    Xf, Wf, b = X.float(), W.float(), bias.float().clone()
    M, N = Xf.shape[0], Wf.shape[0]
    if defect == "neighbour_row":          # the last row of the ragged panel taken from its neighbour
        Xf = Xf.clone()
        Xf[M - 1] = Xf[M - 2]
    acc = Xf @ Wf.t()
    if defect == "drop_k_slab":            # the last K-slab of 64 dropped for the last output tile (128 x 128 or smaller)
        r0, c0 = max(M - 128, 0), N - 128
        acc[r0:, c0:] -= Xf[r0:, K - 64:K] @ Wf[c0:, K - 64:K].t()
    bb = b[None, :].expand(M, N).clone()
    if defect == "bias_shift":             # one 16-feature group reads its bias one column to the right
        bb[:, 16:32] = b[17:33][None, :]
    v = acc + bb
    if epi == R.EPI_RESID32:
        return extra.float() + v
    if epi == R.EPI_PATCH:
        return v + extra.float()
    kind = R.out_kind(dtype, epi)
    if epi == R.EPI_DELTA16 and dtype == "bf16":
        v = v.clamp(-R.F16_MAX, R.F16_MAX)
    if epi == R.EPI_GELU16:
        idx = (torch.round(v.clamp(-5.0, 5.0) * 128.0) + 640).long()
        if defect in ("gelu_interval", "gelu_neighbour"):   # the line of one table interval replaced by another's
            hit = int(idx.flatten()[(v.flatten() + 2.0).abs().argmin()])
            idx = torch.where(idx == hit, idx + (1 if defect == "gelu_neighbour" else 8), idx)
        phi = (TAB_B[idx].double() * v.double() + TAB_A[idx].double()).float()        # one fma
        v = v * phi
    if epi == R.EPI_QGELU16:
        c = torch.tensor(-1.702 * 1.44269504088896340736, dtype=torch.float32)
        v = v * (1.0 / (1.0 + torch.exp2(v * c)))
    return R.rnd(v, kind)


def gemm_selftest(dtype, epi, X, W, bias, K, what, extra=None):
    M = X.shape[0]
    y, bound = R.gemm_ref_and_bound(dtype, epi, X, W, bias, K, extra=extra)
    inside(emulate_gemm(dtype, epi, X, W, bias, K, extra), y, bound, what)
    defects = ["drop_k_slab", "bias_shift"]
    if M >= 2:
        defects.append("neighbour_row")    # a one-row GEMM has no neighbour
    if epi == R.EPI_GELU16:
        defects.append("gelu_interval")
    for d in defects:
        leaves(emulate_gemm(dtype, epi, X, W, bias, K, extra, defect=d), y, bound, f"{what} / {d}")


def reduced_rows(M):
    """At most one full 256-row panel in front of the case's own ragged one."""
    return M if M <= 512 else 256 + (M % 256 or 256)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_grid_bound(dtype):
    full = CS.gemm_inputs(11, "grid." + dtype, dtype, 197 * 3, 768, 768, CPU)
    for M, N, K in CS.gemm_grid_shapes():
        X, W, b = full["X"][:M, :K].contiguous(), full["W"][:N, :K].contiguous(), full["bias"][:N].contiguous()
        gemm_selftest(dtype, R.EPI_STORE16, X, W, b, K, f"{dtype} grid {M}x{N}x{K}")


def test_named_cases_reach_their_kernels_on_an_mi355x():
    """Coverage by the dispatch mirror for the 256 CUs of an MI355X (the GPU test repeats this for the device it runs
    on): the four named shapes take the persistent kernel (ragged / several tiles with non-temporal stores / feature
    groups) and gemm256_kernel, the grid takes gemm128_kernel, and the forced variants the three kernels."""
    for case in CS.gemm_cases(256):
        plan = R.gemm_plan(case["M"], case["N"], case["K"], 256)
        for key, want in case["expect"].items():
            assert plan[key] == want, (case["name"], key, plan)
        assert plan["tiles_per_wg"] >= case.get("min_tiles_per_wg", 1)
    assert all(R.gemm_plan(M, N, K, 256)["kernel"] == "gemm128" for M, N, K in CS.gemm_grid_shapes())
    assert [R.gemm_plan(300, 512, 128, 256, variant=v)["kernel"] for v in (1, 2, 3)] == ["gemm128", "gemm256", "gemm256p"]
    assert R.gemm_plan(13 * 256 + 72, 4096, 1024, 256)["fgroup"] == 4
    assert R.ln_plan(16392, 1024, 0) == "plain_nt" and R.ln_plan(16384, 1024, 0) == "plain"


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_named_and_addressing_bound(dtype):
    for idx, case in enumerate(CS.gemm_cases(8)):
        M, N, K = reduced_rows(case["M"]), case["N"], case["K"]
        ins = CS.gemm_inputs(12 + idx, case["name"] + dtype, dtype, M, N, K, CPU)
        gemm_selftest(dtype, R.EPI_STORE16, ins["X"], ins["W"], ins["bias"], K, f"{dtype} {case['name']}")
    B, T, H = 37, 17, 256
    act = CS.gemm_inputs(60, "addr." + dtype, dtype, B * T, 3 * H, H, CPU)
    Xcls = act["X"][::T].contiguous()
    gemm_selftest(dtype, R.EPI_STORE16, Xcls, act["W"][:H], act["bias"][:H], H, f"{dtype} cls query")
    gemm_selftest(dtype, R.EPI_DELTA16, Xcls, act["W"][:H], act["bias"][:H], H, f"{dtype} cls rows")
    gemm_selftest(dtype, R.EPI_STORE16, act["X"], act["W"][H:], act["bias"][H:], H, f"{dtype} kv only")
    fc1 = CS.gemm_inputs(61, "addr.fc1." + dtype, dtype, B * T, 256, 64, CPU, z_std=2.5)
    for epi in (R.EPI_GELU16, R.EPI_QGELU16):
        gemm_selftest(dtype, epi, fc1["X"][::T].contiguous(), fc1["W"], fc1["bias"], 64, f"{dtype} cls rows fc1 {EPI_NAME[epi]}")
    fc2 = CS.gemm_inputs(62, "addr.fc2." + dtype, dtype, B * T, 128, 256, CPU)
    gemm_selftest(dtype, R.EPI_DELTA16, fc2["X"][::T].contiguous(), fc2["W"], fc2["bias"], 256, f"{dtype} cls rows fc2")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_epilogue_bounds(dtype):
    shapes = {"gemm128": (197 * 3, 256, 64), "gemm256p": (reduced_rows(CS.gemm_cases(8)[0]["M"]), 256, 64)}
    for which, (M, N, K) in shapes.items():
        ins = CS.gemm_inputs(20, f"epi.{which}.{dtype}", dtype, M, N, K, CPU, z_std=2.5)
        for epi in (0, 5, 1, 2):
            gemm_selftest(dtype, epi, ins["X"], ins["W"], ins["bias"], K, f"{dtype} {which} {EPI_NAME[epi]}")
        resid = CS.t32(CS.syn.normal(21, "epi.resid", (M, N), std=4.0), CPU)
        gemm_selftest(dtype, R.EPI_RESID32, ins["X"], ins["W"], ins["bias"], K, f"{dtype} {which} RESID32", extra=resid)
    for P in (196, 576):
        M, N, K = 3 * P, 256, 64
        ins = CS.gemm_inputs(30, f"patch.gemm128.{dtype}.{P}", dtype, M, N, K, CPU)
        pos = CS.t32(CS.syn.normal(31, f"patch.pos.{P}", (P + 1, N), std=1.0), CPU)
        gemm_selftest(dtype, R.EPI_PATCH, ins["X"], ins["W"], ins["bias"], K, f"{dtype} PATCH {P}",
                      extra=pos[1:1 + P].repeat(3, 1))
    ins = CS.gemm_inputs(40, "variants." + dtype, dtype, 300, 512, 128, CPU, z_std=2.5)
    for epi in (0, 5, 1, 2):
        gemm_selftest(dtype, epi, ins["X"], ins["W"], ins["bias"], 128, f"{dtype} variants {EPI_NAME[epi]}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("epi", (R.EPI_GELU16, R.EPI_QGELU16))
def test_activation_sweep_bound(dtype, epi):
    """The dense sweep: every value of the type in [-6, 6].  The pre-activation is exact here, so the bound is u_out plus
    the activation's own documented error - and a table line taken from the neighbouring interval must leave it."""
    ins = CS.gelu_sweep_inputs(dtype, CPU)
    y, bound = R.gemm_ref_and_bound(dtype, epi, ins["X"], ins["W"], ins["bias"], 64, exact_pre=True)
    inside(emulate_gemm(dtype, epi, ins["X"], ins["W"], ins["bias"], 64), y, bound, f"{dtype} sweep {EPI_NAME[epi]}")
    if epi == R.EPI_GELU16:
        leaves(emulate_gemm(dtype, epi, ins["X"], ins["W"], ins["bias"], 64, defect="gelu_interval"), y, bound,
               f"{dtype} sweep / gelu_interval")
        # WHY the planted table defect takes the line of the interval 8 places on (1/16 away) and not the immediate
        # neighbour's: a chord line of Phi over an interval of width h, carried 1.5 h into the next one, is off by at most
        # (1.5 h)^2 / 2 max |Phi''| = 1.125 h^2 * 0.242 = 1.7e-5 there, so adjacent lines differ by no more than that plus
        # their own two errors (h^2 / 16 max |Phi''| each): twenty times below the half ulp of an fp16 store at Phi ~ 0.5.
        # No per-element test of a 16-bit output can be asked to see it.  The gap is computed, so the choice is checked.
        xs = torch.linspace(-4.9, 4.9, 100001, dtype=torch.float64)
        i0 = (torch.round(xs * 128.0) + 640).long()
        gap = ((TAB_A[i0 + 1].double() + TAB_B[i0 + 1].double() * xs) - (TAB_A[i0].double() + TAB_B[i0].double() * xs)).abs()
        h2 = R.GELU_TAB_H ** 2 * 0.242          # 0.242 = max |Phi''| = phi(1)
        assert float(gap.max()) <= (1.125 + 2.0 / 16.0) * h2 + 4.0 * R.U32   # + the entries' fp32 storage, |a| + |b x| <= 2
        # the table restated here meets the two statements of context.hip it is held to
        x = torch.linspace(-4.99, 4.99, 200001, dtype=torch.float64)
        idx = (torch.round(x * 128.0) + 640).long()
        err = (x * (TAB_A[idx].double() + TAB_B[idx].double() * x) - R.gelu64(x)).abs()
        # + the fp32 storage of the entries, as stage_ref charges it: U32 (|a| + |b x|) |x| <= U32 (1 + 0.8 |x|) |x|
        assert bool((err <= 1.0e-6 * x.abs() + R.U32 * (1.0 + 0.8 * x.abs()) * x.abs()).all())
        far = torch.tensor([5.0 - 1.0 / 256, 5.0, 6.0, 20.0], dtype=torch.float64)
        assert bool(((far - R.gelu64(far)).abs() <= 1.5e-6).all()) and bool((R.gelu64(-far).abs() <= 1.5e-6).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_delta16_range_emulation(dtype):
    """The counterpart of the GPU range case: bias columns +1e5 / -1e5 / NaN.  bf16 encoder: saturation at +-65504, NaN
    kept; fp16 encoder (EPI_DELTA16 is EPI_STORE16): +-inf, NaN kept; every other column inside the ordinary bound."""
    M, N, K = 130, 256, 64
    ins = CS.gemm_inputs(50, f"sat.gemm128.{dtype}", dtype, M, N, K, CPU)
    bias = ins["bias"].clone()
    bias[0], bias[1], bias[2] = 1e5, -1e5, float("nan")
    got = emulate_gemm(dtype, R.EPI_DELTA16, ins["X"], ins["W"], bias, K)
    big = R.F16_MAX if dtype == "bf16" else float("inf")
    assert bool((got[:, 0] == big).all()) and bool((got[:, 1] == -big).all()) and bool(torch.isnan(got[:, 2]).all())
    y, bound = R.gemm_ref_and_bound(dtype, R.EPI_DELTA16, ins["X"], ins["W"], ins["bias"], K)
    inside(got[:, 3:], y[:, 3:], bound[:, 3:], f"{dtype} DELTA16 range")
    # the reference of a saturated column is the clamp itself, and a NaN reference is never "inside"
    ys, bs = R.gemm_ref_and_bound(dtype, R.EPI_DELTA16, ins["X"], ins["W"], bias, K)
    if dtype == "bf16":
        assert bool((ys[:, 0] == R.F16_MAX).all()) and R.worst_ratio(got[:, :2], ys[:, :2], bs[:, :2])[1] == 0
    assert R.worst_ratio(got[:, 2], ys[:, 2], bs[:, 2])[1] == M


# ======================================================================================================================
# attention
# ======================================================================================================================
def emulate_attention(dtype, q, k, v, causal, defect=None):
    """fp32: scores by torch's matmul, exp2 of the scaled difference to the row maximum, the UNROUNDED probabilities
    summed, the rounded ones multiplied with V, division by the sum, one rounding to fp32 and one to 16 bit."""
    qf, kf, vf = q.float(), k.float(), v.float()
    Tq, T = qf.shape[1], kf.shape[1]
    if defect == "key_beyond_T":           # the first slot past T (a re-read of row T - 1) left unmasked
        kf, vf = torch.cat([kf, kf[:, -1:]], 1), torch.cat([vf, vf[:, -1:]], 1)
    s = qf @ kf.transpose(1, 2)
    i = torch.arange(Tq)[:, None]
    j = torch.arange(kf.shape[1])[None, :]
    mask = torch.zeros(Tq, kf.shape[1], dtype=torch.bool)
    if causal:
        mask = j > i
        if defect == "key_beyond_T":
            mask = mask & (j < T)
        if defect == "causal_leak":        # one key j = i + 1 unmasked (rows that have one)
            mask = mask & ~(j == i + 1)
        if defect == "last_key_masked":    # the last valid key of every row: j = i
            mask = mask | (j == i)
    elif defect == "last_key_masked":
        mask = mask | (j == T - 1)
    s = s.masked_fill(mask[None], float("-inf"))
    scale = 0.125 * (1.0 + 2.0 ** -7 if defect == "scale" else 1.0)
    c = torch.tensor(scale * 1.44269504088896340736, dtype=torch.float32)
    m = s.max(dim=-1, keepdim=True).values
    p = torch.exp2(s * c - m * c)
    tot = p.sum(dim=-1, keepdim=True)
    o = R.rnd(p, dtype) @ vf
    return R.rnd(o * (1.0 / tot), dtype)


def attention_selftest(dtype, T, heads, q_rows, causal, NT):
    qkv = CS.attention_inputs(200 + T, f"attn.{dtype}.1.{T}.{heads}", dtype, 1, T, heads, CPU)
    q, k, v = CS.split_qkv(qkv, 1, T, heads)
    Tq = min(16 * ((q_rows + 15) // 16), T) if q_rows else T
    q = q[:, :Tq]
    c, bound = R.attention_ref_and_bound(dtype, q, k, v, causal, NT)
    what = f"{dtype} T={T} heads={heads} q_rows={q_rows} causal={causal}"
    inside(emulate_attention(dtype, q, k, v, causal), c, bound, what)
    defects = ["last_key_masked"]
    if T > 1:                              # with one key the softmax is 1 whatever the scale, and a slot past T holds a
        defects += ["scale", "key_beyond_T"]   # copy of row T - 1 (attention.hip clamps the row): a second copy of the ONLY key changes nothing
    if causal and Tq > 1:
        defects.append("causal_leak")
    for d in defects:
        leaves(emulate_attention(dtype, q, k, v, causal, defect=d), c, bound, f"{what} / {d}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_bound(dtype):
    ARMS = CS.ATTENTION_ARMS
    for T, (arm, heads_list) in sorted(ARMS.items()):
        plan = R.attention_plan(T, 3, heads_list[0], 256)
        assert plan["arm"] == arm
        for heads in heads_list:
            attention_selftest(dtype, T, heads, 0, False, plan["NT"])
            attention_selftest(dtype, T, heads, 1, False, plan["NT"])
    for T in (1, 16, 17, 77, 80):
        attention_selftest(dtype, T, 4, 0, True, 5)
    arms = {R.attention_plan(T, 3, 4, 256)["arm"] for T in ARMS} | {R.attention_plan(T, 3, 4, 256, q_rows=1)["arm"]
                                                                    for T in ARMS}
    assert arms == {"plain2", "plain5", "plain13", "stream13", "long37_persist_few", "long37_persist_many", "long37_pair12",
                    "long37_exact_persist_few", "long37_exact_persist_many"}


# ======================================================================================================================
# LayerNorm, embed, pool
# ======================================================================================================================
def emulate_ln(v32, gamma, beta, eps, store, defect=None):
    """fp32 two-pass statistics in torch's reduction order; `store` None keeps the fp32 result."""
    H = v32.shape[-1]
    mean = v32.mean(dim=-1, keepdim=True)
    d = v32 - mean
    var = (d * d).sum(dim=-1, keepdim=True) / (H - 1 if defect == "sample_variance" else H)
    rstd = torch.rsqrt(var + (0.0 if defect == "no_eps" else eps))
    out = d * rstd * gamma.float() + beta.float()
    return out if store is None else R.rnd(out, store)


def ln_defects(rows, use_b):
    d = ["sample_variance"]
    if rows >= 3:
        d.append("no_eps")                 # needs the constant row (stage_cases.ln_inputs)
    if use_b:
        d.append("dB_twice")               # a null deltaB16 cannot be folded twice
    return d


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", (256, 512, 768, 1024))
def test_resid_layernorm_bound(dtype, H):
    for rows, (use_a, use_b), eps in itertools.product((1, 7, 8, 9, 3 * 197), ((0, 0), (0, 1), (1, 0), (1, 1)),
                                                       (1e-12, 1e-5)):
        ins = CS.ln_inputs(70 + H // 256, f"ln.{H}.{rows}.1", rows, H, CPU)
        dA, dB = (ins["dA"] if use_a else None), (ins["dB"] if use_b else None)
        y, bound = R.resid_layernorm_ref_and_bound(dtype, ins["x"], dA, dB, ins["gamma"], ins["beta"], eps)
        what = f"{dtype} LN H={H} rows={rows} dA={use_a} dB={use_b} eps={eps}"
        v = R.resid_sum32(ins["x"], dA, dB)
        inside(emulate_ln(v, ins["gamma"], ins["beta"], eps, dtype), y, bound, what)
        for d in ln_defects(rows, use_b):
            vv = v + dB.float() if d == "dB_twice" else v
            leaves(emulate_ln(vv, ins["gamma"], ins["beta"], eps, dtype, defect=d), y, bound, f"{what} / {d}")


@pytest.mark.parametrize("H", (256, 512, 768, 1024))
def test_embed_bound(H):
    for (B, T), eps in itertools.product(((3, 5), (2, 197)), (1e-12, 1e-5)):
        ins = CS.embed_inputs(100 + T, f"embed.{H}.{T}", B, T, H, CPU)
        patch16, cls, pos = ins["patch16"], ins["cls"], ins["pos"]
        v = R.embed_exact32(patch16, cls, pos, B, T)
        y, bound = R.embed_ref_and_bound(patch16, cls, pos, ins["gamma"], ins["beta"], eps, True, B, T)
        what = f"embed H={H} T={T} eps={eps}"
        inside(emulate_ln(v, ins["gamma"], ins["beta"], eps, None), y, bound, what)
        for d in ("sample_variance", "no_eps"):
            leaves(emulate_ln(v, ins["gamma"], ins["beta"], eps, None, defect=d), y, bound, f"{what} / {d}")
        y0, b0 = R.embed_ref_and_bound(patch16, cls, pos, None, None, eps, False, B, T)
        inside(v, y0, b0, what + " (no pre-LN)")


def emulate_pool(dtype, x, dA, dB, gamma, beta, eps, pw, l2, defect=None):
    v = R.resid_sum32(x, dA, dB)
    if defect == "dB_twice":
        v = v + dB.float()
    y = emulate_ln(v, gamma, beta, eps, None, defect=defect)
    r = R.rnd(y, dtype) @ pw.float().t() if pw is not None else y
    if l2:
        r = r * (1.0 / torch.sqrt((r * r).sum(dim=-1, keepdim=True)).clamp_min(1e-12))
    return R.rnd(r, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", (256, 512, 768, 1024))
def test_pool_bound(dtype, H):
    B, T = 4, 7
    ins = CS.ln_inputs(120, f"pool.{H}", B * T, H, CPU)
    prow = torch.tensor([0, 6, 3, 1])
    for proj_dim, l2, with_row, eps in itertools.product((0, 128, 768), (0, 1), (0, 1), (1e-12, 1e-5)):
        pw = CS.t16(CS.syn.normal(121, f"pool.w.{proj_dim}.{H}", (max(proj_dim, 1), H), std=0.05), dtype, CPU) \
            if proj_dim else None
        rows = torch.arange(B) * T + (prow if with_row else 0)
        args = (ins["gamma"], ins["beta"], eps, pw, bool(l2))
        y, bound = R.pool_ref_and_bound(dtype, ins["x"][rows], ins["dA"][rows], ins["dB"][rows], *args)
        what = f"{dtype} pool H={H} proj={proj_dim} l2={l2} row={with_row} eps={eps}"
        inside(emulate_pool(dtype, ins["x"][rows], ins["dA"][rows], ins["dB"][rows], *args), y, bound, what)
        # pooled from row 1 instead of row 0, or from pool_row - 1
        wrong = torch.arange(B) * T + ((prow - 1).clamp_min(0) if with_row else 1)
        leaves(emulate_pool(dtype, ins["x"][wrong], ins["dA"][wrong], ins["dB"][wrong], *args), y, bound,
               what + " / wrong row")
        # sample variance moves every LayerNorm output by 1 / (2 H) of its n g part: visible at the pooled row itself, but
        # behind a projection the 16-bit rounding of its H inputs - summed at its worst case, as an element-wise bound
        # must - is larger than that shift, so there the defect is planted on the LayerNorm cases alone
        for d in ("dB_twice", "no_eps") + (("sample_variance",) if proj_dim == 0 else ()):
            leaves(emulate_pool(dtype, ins["x"][rows], ins["dA"][rows], ins["dB"][rows], *args, defect=d), y, bound,
                   f"{what} / {d}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_zero_row_emulation(dtype):
    """The counterpart of the GPU zero-row case: gamma = beta = 0 makes the pooled vector exactly 0; under l2 = 1 the clamp
    at 1e-12 keeps the result 0 (never NaN), and the reference says 0 as well."""
    B, T, H = 3, 5, 512
    ins = CS.ln_inputs(130, "pool.zero", B * T, H, CPU)
    zero = torch.zeros(H)
    rows = torch.arange(B) * T
    for proj in (False, True):
        pw = CS.t16(CS.syn.normal(131, "pool.zero.w", (128, H), std=0.05), dtype, CPU) if proj else None
        got = emulate_pool(dtype, ins["x"][rows], ins["dA"][rows], ins["dB"][rows], zero, zero, 1e-5, pw, True)
        y, bound = R.pool_ref_and_bound(dtype, ins["x"][rows], ins["dA"][rows], ins["dB"][rows], zero, zero, 1e-5, pw, True)
        assert bool((got == 0).all()) and bool((y == 0).all())
        inside(got, y, bound, f"{dtype} pool zero row proj={proj}")


def test_text_embed_reference():
    """The restatement against a plain loop (the GPU test holds the kernel to bit equality with it)."""
    vocab, eot, B, T, H = 50, 49, 4, 6, 256
    ids = torch.tensor([[49, 1, 2, 3, 4, 5], [1, 2, 49, 3, 49, 4], [-3, 60, 1, 2, 3, 4], [1, 2, 3, 4, 5, 49]], dtype=torch.int32)
    tok = CS.t32(CS.syn.normal(1, "t.tok", (vocab, H)), CPU)
    pos = CS.t32(CS.syn.normal(1, "t.pos", (T, H)), CPU)
    x, row, flags = R.text_embed_exact(ids, tok, pos, vocab, eot)
    for b in range(B):
        for t in range(T):
            i = min(max(int(ids[b, t]), 0), vocab - 1)
            assert torch.equal(x[b, t], tok[i] + pos[t])
    assert row.tolist() == [0, 2, 0, 5] and flags.tolist() == [0, 0, 3, 0]
