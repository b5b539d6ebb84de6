"""fp64 restatements of the encoder's kernel stages, element-wise error bounds, and a mirror of their dispatch.

A test helper, not a conftest.  Every reference takes the exact 16-bit / fp32 buffers the kernel receives (as torch
tensors, on any device) and restates the stage in ``torch.float64``.  Beside each reference stands a bound
``|device - reference| <= bound`` per ELEMENT that is a formula of reference quantities alone: the sum of the rounding
points the kernel really has, read from its code (cited in each docstring).  No tolerance here is a bare constant and
none comes from a device result.  tests/test_stage_ref_cpu.py proves each bound before it judges a kernel: an
independent fp32 emulation must lie inside on every element, and each of a list of planted defects must leave it.

Units: U32 = 2^-24 (fp32 round to nearest), u_out = 2^-11 (fp16 store) / 2^-8 (bf16 store).  One MFMA or intrinsic
step whose rounding mode the ISA does not spell out as round-to-nearest is charged 1 ulp = 2 U32.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

U32 = 2.0 ** -24
U_OUT = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
# half the smallest subnormal of the store type: the absolute rounding error where the relative one stops holding
HALF_SUB = {"f16": 2.0 ** -25, "bf16": 2.0 ** -134}
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
F16_MAX = 65504.0

EPI_STORE16, EPI_GELU16, EPI_QGELU16, EPI_RESID32, EPI_PATCH, EPI_DELTA16 = 0, 1, 2, 3, 4, 5
OUT16_EPIS = (EPI_STORE16, EPI_DELTA16, EPI_GELU16, EPI_QGELU16)


def out_kind(dtype: str, epi: int) -> str:
    """Storage type of a 16-bit epilogue: EPI_DELTA16 is fp16 whatever the encoder's dtype (csrc/vm_kernels.h)."""
    return "f16" if epi == EPI_DELTA16 else dtype


def rnd(x: torch.Tensor, kind: str) -> torch.Tensor:
    """Round an fp32 tensor to the 16-bit type and back (the device's v_cvt_pk: RNE), as oracle/vit_ref's rounders do."""
    return x.to(TDT[kind]).to(torch.float32)


def gamma_n(n: float) -> float:
    """n roundings of U32 compounded: n u / (1 - n u)."""
    return n * U32 / (1.0 - n * U32)


# ======================================================================================================================
# dispatch mirrors (in the manner of tests/topk_plan.py): which kernel a call takes for the device's CU count
# ======================================================================================================================
def gemm_tile_addressable(K: int, ldx: int) -> bool:
    """csrc/gemm_guard.h vm_gemm256_tile_addressable."""
    lim = 1 << 31
    if K <= 0 or ldx < K:
        return False
    return 256 * K * 2 < lim and (255 * ldx + K) * 2 < lim


def gemm_plan(M: int, N: int, K: int, num_cus: int, ldx: Optional[int] = None, variant: int = 0) -> Dict:
    """csrc/gemm.hip launch_epi (kernel choice) and vm_gemm (stream_out, fgroup) of the release build."""
    ldx = K if ldx is None else ldx
    assert M > 0 and N % 128 == 0 and K % 64 == 0 and K > 0
    tiles256 = ((M + 255) // 256) * (N // 256)
    big_ok = N % 256 == 0 and gemm_tile_addressable(K, ldx)
    if variant in (2, 3):
        use256 = big_ok
    elif variant == 1:
        use256 = False
    else:
        use256 = big_ok and tiles256 * 10 >= num_cus * 8
    if use256 and variant != 2 and N <= 4096:
        kernel, grid = "gemm256p", min(tiles256, num_cus)
    elif use256:
        kernel, grid = "gemm256", tiles256
    else:
        kernel, grid = "gemm128", ((M + 127) // 128) * (N // 128)
    stream_out = M * N * 2 > (32 << 20)
    fgroup = 0
    budget = 2560 * 1024
    tiles_n = N // 256
    wtile = 256 * K * 2
    wall = wtile * tiles_n
    if N % 256 == 0 and wall > budget and wtile <= budget:
        ngroups = (wall + budget - 1) // budget
        fg = (tiles_n + ngroups - 1) // ngroups
        ng = (tiles_n + fg - 1) // fg
        x_extra = float(ng - 1) * M * K * 2
        rounds = float((M + 255) // 256) * tiles_n / num_cus
        if x_extra < rounds * 8.0 * wall:
            fgroup = fg
    # the persistent kernel alone reads fgroup, and only a value below tiles_n changes its tile order
    fgroup_active = kernel == "gemm256p" and 0 < fgroup < tiles_n
    return dict(kernel=kernel, grid=grid, tiles256=tiles256, stream_out=stream_out, fgroup=fgroup,
                fgroup_active=fgroup_active,
                tiles_per_wg=(tiles256 + grid - 1) // grid if kernel == "gemm256p" else 1)


def ln_plan(rows: int, H: int, lowreg: int) -> str:
    """csrc/encoder.hip vm_resid_layernorm: the low-register build (always streaming), else by the 64 MiB rule."""
    assert H % 256 == 0 and 256 <= H <= 1024
    if lowreg:
        return "lowreg_nt"
    return "plain_nt" if rows * H * 4 > (64 << 20) else "plain"


def attention_plan(T: int, B: int, heads: int, num_cus: int, q_rows: int = 0, causal: int = 0) -> Dict:
    """csrc/attention.hip dispatch / launch_long of the release build."""
    nt = (T + 15) // 16
    if causal:
        assert nt <= 5
        return dict(arm="causal5", NT=5, exact=False, ql=5)
    ql = (q_rows + 15) // 16 if q_rows > 0 else nt
    items = B * heads
    if nt == 13:
        return dict(arm="stream13", NT=13, exact=True, ql=min(ql, 13), grid=min(items, num_cus),
                    items_per_wg=(items + min(items, num_cus) - 1) // min(items, num_cus))
    if nt == 37 or 13 < nt <= 37:
        exact = nt == 37
        qlc = min(ql, 37)
        npairs = (qlc + 1) // 2
        maxc = (npairs + 11) // 12
        w0 = npairs - (maxc - 1) * 12
        if w0 >= 12:
            w0 = 0
        groups = 2 * 37 * 16 // 8
        pf = (groups + (12 - w0) - 1) // (12 - w0)
        if pf <= (groups + 10) // 11:
            sub = "persist_many"
        elif pf <= (groups + 4) // 5:
            sub = "persist_few"
        else:
            sub = "pair12"
        return dict(arm=("long37_exact_" if exact else "long37_") + sub, NT=37, exact=exact, ql=qlc,
                    grid=min(items, num_cus) if sub != "pair12" else items)
    if nt <= 2:
        return dict(arm="plain2", NT=2, exact=False, ql=min(ql, 2))
    if nt <= 5:
        return dict(arm="plain5", NT=5, exact=False, ql=min(ql, 5))
    assert nt <= 13
    return dict(arm="plain13", NT=13, exact=False, ql=min(ql, 13))


# ======================================================================================================================
# GEMM + epilogues
# ======================================================================================================================
GELU_LIP = 1.13     # max |d/dx x Phi(x)| = 1.1290 (at |x| = 1.414)
QGELU_LIP = 1.10    # max |d/dx x sigmoid(1.702 x)| = 1.0998
GELU_TAB_H = 1.0 / 128.0


def gelu64(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * torch.special.erfc(-x * 0.70710678118654752440)


def qgelu64(x: torch.Tensor) -> torch.Tensor:
    return x * torch.sigmoid(1.702 * x)


def gemm_pre(X: torch.Tensor, W: torch.Tensor, bias: torch.Tensor):
    """z = X W^T + b and A = |X| |W|^T + |b| in fp64 (X [M, K] and W [N, K] 16-bit, bias fp32)."""
    Xd, Wd, bd = X.double(), W.double(), bias.double()
    return Xd @ Wd.t() + bd, Xd.abs() @ Wd.abs().t() + bd.abs()


def gemm_acc_err(A: torch.Tensor, K: int) -> torch.Tensor:
    """|fl32(acc + bias) - z| <= gamma(2 (K + 1)) A.

    gemm.hip: every kernel chains K/32 MFMA 16x16x32 through one fp32 accumulator and adds the fp32 bias once (v_pk_add).
    Products of two 16-bit operands are exact in fp32 (<= 22 significant bits).  An output therefore passes through K
    additions inside the matrix unit, whose rounding the ISA does not state to be round-to-nearest: 1 ulp = 2 U32 each
    (the constant c = 2 of the bound), and one more for the bias add.  All partial sums are bounded by A."""
    return gamma_n(2.0 * (K + 1)) * A


def gemm_ref_and_bound(dtype: str, epi: int, X, W, bias, K: int, extra: Optional[torch.Tensor] = None,
                       exact_pre: bool = False):
    """(y, bound) of one GEMM epilogue; ``extra`` is the fp32 residual (EPI_RESID32) or position row (EPI_PATCH) per
    output element.

    Common part: v = fl32(acc + b), |v - z| <= E = gemm_acc_err.
    STORE16 / DELTA16 (epilogue_row / epilogue16: pack2 = one RNE conversion; DELTA16 of a bf16 encoder first clamps to
      +-65504, a 1-Lipschitz map that keeps NaN):  y = z (clamped), |got - y| <= E + u_out (|y| + E) + half_sub.
    GELU16 (table, gelu_tab_addr / gelu_tab_apply4): got = rn16(fl(v * fl(fma(b_i, v, a_i)))).  context.hip states
      |x Phi(x) - x (a + b x)| <= 1.0e-6 |x| inside the table and 1.5e-6 beyond |x| >= 5 - h/2; the kernel is held to
      those two statements.  Evaluation in fp32: the entries are floats (|a| <= 1 + 0.4 |x|, |b| <= 0.4: U32 (1 + 0.8 |x|)
      on Phi), one fma and one product (2 U32 on values <= |x|): U32 |x| (3 + 0.8 |x|).  The pre-activation error E
      passes through at the Lipschitz constant 1.13 of x Phi(x).
    QGELU16 (quick_gelu): t = fl(x c) with c = fl(-1.702 log2 e) (2 U32 |t|), e = v_exp_f32(t) (1 ulp = 2 U32, plus the
      argument error times ln 2), 1 + e (U32), v_rcp_f32 (1 ulp = 2 U32), product (U32): relative error of the sigmoid
      s <= (1 - s) 2 U32 (1 + |t| ln 2) + 3 U32, of y one U32 more.  Lipschitz constant 1.10.
    RESID32: out = fl32(r + v): |got - (r + z)| <= E + U32 (|r + z| + E).   PATCH: out = fl32(v + pos): the same.
    exact_pre: the caller has built operands whose sums hold ONE non-zero product and a zero bias (the dense activation
      sweep): every partial sum is that product or 0, exact in fp32, so E = 0 and the activation is held to u_out plus
      its own documented error alone.
    """
    z, A = gemm_pre(X, W, bias)
    E = torch.zeros_like(A) if exact_pre else gemm_acc_err(A, K)
    if epi in (EPI_RESID32, EPI_PATCH):
        y = z + extra.double()
        return y, E + U32 * (y.abs() + E)
    kind = out_kind(dtype, epi)
    u, hs = U_OUT[kind], HALF_SUB[kind]
    if epi == EPI_STORE16 or epi == EPI_DELTA16:
        y = z.clamp(-F16_MAX, F16_MAX) if (epi == EPI_DELTA16 and dtype == "bf16") else z
        pre = E
    elif epi == EPI_GELU16:
        y = gelu64(z)
        az = z.abs()
        inside = 1.0e-6 * (az + E)
        beyond = torch.where(az + E >= 5.0 - GELU_TAB_H / 2, torch.full_like(az, 1.5e-6), torch.zeros_like(az))
        pre = GELU_LIP * E + torch.maximum(inside, beyond) + U32 * (az + E) * (3.0 + 0.8 * (az + E))
    elif epi == EPI_QGELU16:
        y = qgelu64(z)
        s = torch.sigmoid(1.702 * z)
        t = (1.702 * 1.44269504088896340736) * z.abs()
        rel = (1.0 - s) * 2.0 * U32 * (1.0 + t * math.log(2.0)) + 4.0 * U32
        pre = QGELU_LIP * E + rel * y.abs()
    else:
        raise ValueError(epi)
    return y, pre + u * (y.abs() + pre) + hs


def gelu_table():
    """The context's erf-GELU table restated (context.hip build_gelu_table): fp32 pairs {a, b}, 1,281 entries."""
    n, h = 1281, GELU_TAB_H
    i = torch.arange(n, dtype=torch.float64)
    xc = -5.0 + i * h
    lo, hi = xc - 0.5 * h, xc + 0.5 * h
    Phi = lambda x: 0.5 * torch.special.erfc(-x * 0.70710678118654752440)
    b = (Phi(hi) - Phi(lo)) / (hi - lo)
    j = torch.arange(65, dtype=torch.float64) / 64.0
    xs = lo[:, None] + (hi - lo)[:, None] * j[None, :]
    d = Phi(xs) - b[:, None] * xs
    a = 0.5 * (d.min(dim=1).values + d.max(dim=1).values)
    a[0], b[0], a[-1], b[-1] = 0.0, 0.0, 1.0, 0.0
    return a.float(), b.float()


# ======================================================================================================================
# attention
# ======================================================================================================================
def attention_ref_and_bound(dtype: str, q, k, v, causal: bool, NT: int):
    """softmax(q k^T / 8) v per (batch, head): q [G, Tq, 64], k / v [G, T, 64] 16-bit.  Returns (c, bound) [G, Tq, 64].

    attention.hip attend_tile / attend_tile_pass2 / the pair walks.  Which sum normalises: the fp32 sum of the UNROUNDED
    probabilities p_j (sum2 adds the v_exp results); the P.V product uses p_j rounded to the encoder's 16-bit type.
    With p_j = p*_j (1 + eta_j) (fp32 effects) and rn16(p_j) = p_j (1 + rho_j), |rho_j| <= u_p:
        got' = sum_j p*_j (1 + eta_j)(1 + rho_j) v_j / sum_j p*_j (1 + eta_j)
        |got' - c| <= u_p (P |V|) + (P o eta) |V| + rowsum(P o eta) |c|          (first order; P = fp64 probabilities)
    so the 16-bit rounding of P enters once (numerator only) and the fp32 effects twice.  eta_j, from the code:
      score: 64 products through two chained MFMAs, 2 U32 per addition (as gemm_acc_err): Es_j = gamma(2 * 64) |q|.|k_j|,
             times (1/8) (the shift by the row reference cancels between numerator and denominator, its rounding too);
      argument: one fma s * c + n with c = fl(log2(e) / 8): 2 U32 |arg_j|, |arg_j| <= |s_j - max| log2(e) / 8 + 6 (the
             online walks keep a lazily raised reference up to 2^6 below the row maximum);
      v_exp_f32: 1 ulp = 2 U32.
      eta_j = ln 2 (log2(e) / 8 Es_j + 2 U32 |arg_j|) + 2 U32.
    A probability below fp16's normal range is rounded with ABSOLUTE error 2^-25; it is scaled by <= 1 afterwards and
    the normalising sum is >= 1 (the row maximum contributes >= 1): + 2^-25 sum_j |v_j| for fp16.
    Further fp32 steps, all relative to P |V|: the P.V accumulation over 16 NT key slots (2 U32 each), the sum of the
    probabilities (<= 2 NT + 3 additions), up to NT / 2 rescales of both (U32 each, the factor itself cancels), the
    division and the product (ctx_value: product rounded to fp32, THEN to 16 bit): (32 NT + 2 NT + 3 + NT + 2) U32.
    Store: u_out (|c| + all of the above) + half_sub.
    """
    qd, kd, vd = q.double(), k.double(), v.double()
    Tq, T = q.shape[1], k.shape[1]
    s = qd @ kd.transpose(1, 2)
    sa = qd.abs() @ kd.abs().transpose(1, 2)
    if causal:
        i = torch.arange(Tq, device=q.device)[:, None]
        j = torch.arange(T, device=q.device)[None, :]
        s = s.masked_fill(j > i, float("-inf"))
    m = s.max(dim=-1, keepdim=True).values
    P = torch.softmax(s / 8.0, dim=-1)
    c = P @ vd
    PV = P @ vd.abs()
    l2e = 1.44269504088896340736
    arg = torch.where(torch.isfinite(s), (m - s) * (l2e / 8.0) + 6.0, torch.zeros_like(s))
    eta = math.log(2.0) * (l2e / 8.0 * gamma_n(128.0) * sa + 2.0 * U32 * arg) + 2.0 * U32
    Pe = P * eta
    u, hs = U_OUT[dtype], HALF_SUB[dtype]
    pre = u * PV + Pe @ vd.abs() + Pe.sum(dim=-1, keepdim=True) * c.abs() + (35.0 * NT + 5.0) * U32 * PV
    if dtype == "f16":
        va = vd.abs()
        if causal:
            pre = pre + 2.0 ** -25 * torch.cumsum(va, dim=1)[:, :Tq]
        else:
            pre = pre + 2.0 ** -25 * va.sum(dim=1, keepdim=True)
    return c, pre + u * (c.abs() + pre) + hs


# ======================================================================================================================
# residual add + LayerNorm, embed, pool, text embed
# ======================================================================================================================
def resid_sum32(x32, dA, dB):
    """v = (x32 + dA) + dB as the kernels form it: two fp32 additions in that order (IEEE: torch gives the same bits)."""
    v = x32.float()
    if dA is not None:
        v = v + dA.float()
    if dB is not None:
        v = v + dB.float()
    return v


def _ln_stat_counts(H: int):
    """Roundings of the two-pass statistics of one wave per row (encoder.hip resid_layernorm_kernel, both builds, and
    embed_kernel), VPL = H / 256 float4 per lane:
      mean: (x + y) + (z + w) = 2 additions deep, VPL additions into the lane's sum, 6 DPP additions (wave_sum), one
            division: VPL + 9, relative to mean |v|;
      var + eps: d = v - mean (U32, doubled by the square), the square (U32), 2 additions deep, VPL, 6, the division,
            the + eps: VPL + 13, relative (every term is >= 0)."""
    vpl = H // 256
    return vpl + 9.0, vpl + 13.0


def _pool_stat_counts(H: int):
    """pool_kernel: H / 256 additions per thread, 6 (wave_sum), 2 (the four wave sums), one division: + 9; the variance
    as above without the pairwise step: d (2 U32), square, H / 256, 6, 2, division, + eps = H / 256 + 13."""
    vpl = H // 256
    return vpl + 9.0, vpl + 13.0


def layernorm_ref_and_bound(v64: torch.Tensor, e_in: torch.Tensor, gamma, beta, eps: float, counts,
                            store: Optional[str]):
    """y = LN(v) * gamma + beta in fp64 over the last axis, and the bound of the kernels' fp32 evaluation.

    v64: the exact row (fp64 sum of the inputs); e_in: bound of |v_kernel - v64| per element (the fp32 additions that
    formed the row).  With n = (v - mu) rstd (population variance, rstd = 1 / sqrt(var + eps)):
      input error, first order and exact in form:  |g| rstd (e_i + mean(e) + |n_i| mean(|n| e))
      mean in fp32 (counts[0] = c_mu roundings):   |d mu| <= gamma(c_mu) mean |v|  ->  |g| rstd |d mu|; the variance
            taken around the shifted mean grows by d mu^2: relative (d mu rstd)^2 / 2 on rstd
      var + eps (counts[1] = c_var): relative c_var U32, halved by the square root; rsqrtf: 1 ulp = 2 U32
      output: d = fl(v - mean) (U32), d * rstd (U32), * gamma (U32) -> 3 U32 on |n g|; + beta: U32 |y|
      store (resid_layernorm: rn16; embed's pre-LN: fp32, nothing more): u_out (|y| + everything above) + half_sub.
    """
    g, b = gamma.double(), beta.double()
    mu = v64.mean(dim=-1, keepdim=True)
    d = v64 - mu
    var = (d * d).mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    n = d * rstd
    y = n * g + b
    c_mu, c_var = counts
    e_mean = e_in.mean(dim=-1, keepdim=True)
    t_in = g.abs() * rstd * (e_in + e_mean + n.abs() * (n.abs() * e_in).mean(dim=-1, keepdim=True))
    dmu = gamma_n(c_mu) * (v64.abs() + e_in).mean(dim=-1, keepdim=True)
    rel_rstd = 0.5 * gamma_n(c_var) + 2.0 * U32 + 0.5 * (dmu * rstd) ** 2
    pre = t_in + g.abs() * rstd * dmu + (n * g).abs() * (rel_rstd + 3.0 * U32) + U32 * y.abs()
    if store is None:
        return y, pre
    return y, pre + U_OUT[store] * (y.abs() + pre) + HALF_SUB[store]


def resid_exact_and_err(x32, dA, dB):
    """(v64, e_in): the exact fp64 row and the bound of the kernel's two fp32 additions, U32 per addition on its result."""
    v64 = x32.double()
    e = torch.zeros_like(v64)
    if dA is not None:
        v64 = v64 + dA.double()
        e = e + U32 * v64.abs()
    if dB is not None:
        v64 = v64 + dB.double()
        e = e + U32 * (v64.abs() + e)
    return v64, e


def resid_layernorm_ref_and_bound(dtype, x32, dA, dB, gamma, beta, eps):
    v64, e = resid_exact_and_err(x32, dA, dB)
    return layernorm_ref_and_bound(v64, e, gamma, beta, eps, _ln_stat_counts(x32.shape[-1]), dtype)


def embed_ref_and_bound(patch16, cls, pos, pre_g, pre_b, eps, pre_ln: bool, B: int, T: int):
    """x32[b*T + t] = (t ? patch16[b*(T-1) + t-1] : cls) + pos[t] (one fp32 addition; patch rows are fp16 whatever the
    encoder's dtype), then the optional pre-LayerNorm with an fp32 result.  Without pre-LN the stage is fully determined:
    the caller compares with embed_exact32 bit for bit."""
    H = pos.shape[-1]
    e = torch.cat([cls.double()[None, None, :].expand(B, 1, H), patch16.double().view(B, T - 1, H)], dim=1)
    v64 = e + pos.double()[None]
    err = U32 * v64.abs()
    if not pre_ln:
        return v64, err
    return layernorm_ref_and_bound(v64, err, pre_g, pre_b, eps, _ln_stat_counts(H), None)


def embed_exact32(patch16, cls, pos, B: int, T: int):
    H = pos.shape[-1]
    e = torch.cat([cls.float()[None, None, :].expand(B, 1, H), patch16.float().view(B, T - 1, H)], dim=1)
    return e + pos.float()[None]


def pool_ref_and_bound(dtype, xrow, dArow, dBrow, gamma, beta, eps, proj_w, l2: bool):
    """The pooled row of each sequence ([B, H] slices of x / delta16 / deltaB16 at the pooled row) -> final LayerNorm,
    optional projection, optional L2 normalisation, 16-bit store (encoder.hip pool_kernel).

      LayerNorm in fp32, result y kept in fp32 (LDS): layernorm_ref_and_bound without a store -> e_y.
      projection: r_o = sum_i rn16(y_i) w_oi, fp32: the 16-bit rounding of y (u_in (|y| + e_y)), H / 64 additions per
        lane + 6 (wave_sum) + 1 (the product) roundings of U32 on sum |y| |w|:
        e_r = (e_y + u_in (|y| + e_y)) |W|^T + gamma(H / 64 + 7) (|y| |W|^T).
      L2: nn = sum r^2 in fp32 (out_dim / 256 + 10 roundings, relative), sqrtf and the division correctly rounded, the
        clamp fmaxf(nrm, 1e-12): out = r / max(|r|, 1e-12).  CONTRACT of a zero row: nn = 0 -> inv = 1e12 -> every
        output is 0 * 1e12 = 0 exactly (never NaN); the reference applies the same clamp.
        d(r / N) <= e_r / N + |r| / N (|e_r| . |r| / N^2 + gamma(c) ) with N the clamped norm;  then the product (U32).
      store: u_out (|out| + everything above) + half_sub.
    """
    H = xrow.shape[-1]
    v64, e = resid_exact_and_err(xrow, dArow, dBrow)
    y, e_y = layernorm_ref_and_bound(v64, e, gamma, beta, eps, _pool_stat_counts(H), None)
    if proj_w is not None:
        Wd = proj_w.double()
        e_in = e_y + U_OUT[dtype] * (y.abs() + e_y) + HALF_SUB[dtype]
        r = y @ Wd.t()
        e_r = e_in @ Wd.abs().t() + gamma_n(H / 64.0 + 7.0) * ((y.abs() + e_in) @ Wd.abs().t())
    else:
        r, e_r = y, e_y
    if l2:
        od = r.shape[-1]
        nrm = torch.sqrt((r * r).sum(dim=-1, keepdim=True))
        N = nrm.clamp_min(1e-12)
        out = r / N
        d_rel = ((e_r * r.abs()).sum(dim=-1, keepdim=True) / (N * N)) + gamma_n(od / 256.0 + 10.0) + 3.0 * U32
        pre = e_r / N + out.abs() * d_rel + U32 * out.abs()
        # second order, needed only where e_r is not small against the norm (a zero row): the norm moves by <= |e_r|_2
        pre = pre + (e_r / N) * (torch.sqrt((e_r * e_r).sum(dim=-1, keepdim=True)) / N)
    else:
        out, pre = r, e_r
    return out, pre + U_OUT[dtype] * (out.abs() + pre) + HALF_SUB[dtype]


def text_embed_exact(ids, tok, pos, vocab: int, eot_id: int):
    """Fully determined (encoder.hip text_embed_kernel): x32 = tok[clamp(id)] + pos[t] (one fp32 addition),
    pool_row = first t with id == eot_id else 0, flags = bit 0 (an id was clamped) | bit 1 (no EOT)."""
    B, T = ids.shape
    idc = ids.clamp(0, vocab - 1).long()
    x = tok.float()[idc] + pos.float()[None, :T]
    hit = ids == eot_id
    has = hit.any(dim=1)
    first = torch.where(has, hit.int().argmax(dim=1), torch.zeros(B, dtype=torch.long, device=ids.device))
    clamped = ((ids < 0) | (ids >= vocab)).any(dim=1)
    flags = clamped.int() + 2 * (~has).int()
    return x, first.int(), flags.int()


def worst_ratio(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor):
    """(max error / bound, count of elements outside).  A NaN on either side counts as outside: no element is excluded."""
    err = (got.double() - ref).abs()
    ok = err <= bound
    ratio = torch.where(torch.isfinite(err), err / bound, torch.full_like(err, float("inf")))
    return float(ratio.max()), int((~ok).sum())
