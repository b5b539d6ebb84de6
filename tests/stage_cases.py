"""Case tables and seeded inputs of the stage tests (tests/test_stage_*_gpu.py, tests/test_stage_ref_cpu.py).

A test helper, not a conftest.  The GPU tests run every case at full size; the CPU self-test of the bounds runs the SAME
case list at reduced size (``gemm_cases(num_cus=8)``: the CU-count-dependent row counts shrink with the pretended chip;
attention and LayerNorm cases keep their shapes and take fewer sequences / rows).  Shapes are the smallest that reach
the named kernel path; tests/stage_ref.py's dispatch mirror says which path that is.
"""
from __future__ import annotations

import math
from typing import Dict, List

import numpy as np
import torch

from vidmem import synthetic as syn

import tests.stage_ref as R

CANARY16 = 0x7E7E          # fp16: a NaN; bf16: 5.3e37 - either way nothing a kernel computes here
CANARY32 = 0x7FC0DEAD      # fp32: a NaN
NAN16 = 0x7FFF             # a NaN in fp16 AND in bf16: the fill around a 16-bit OPERAND (a read past it shows in the result)
GUARD_ROWS = 512


def t16(a: np.ndarray, dtype: str, device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(device).to(R.TDT[dtype])


def t32(a: np.ndarray, device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def canary16(rows: int, cols: int, device) -> torch.Tensor:
    return torch.full((rows, cols), CANARY16, dtype=torch.int16, device=device)


def canary32(rows: int, cols: int, device) -> torch.Tensor:
    return torch.full((rows, cols), CANARY32, dtype=torch.int32, device=device)


def untouched(buf: torch.Tensor) -> bool:
    """Every element of an integer view still holds the canary."""
    c = CANARY16 if buf.dtype == torch.int16 else CANARY32
    return bool((buf == c).all())


# ======================================================================================================================
# GEMM
# ======================================================================================================================
def gemm_grid_shapes():
    """gemm128_kernel's own edges: one row, a partial 16-row MFMA block, one short of / exactly / one past a 128-row tile,
    several ragged tiles; one, three and six feature tiles; one, two and twelve K-tiles."""
    return [(M, N, K) for M in (1, 3, 127, 128, 129, 197 * 3) for N in (128, 384, 768) for K in (64, 128, 768)]


def gemm_cases(num_cus: int) -> List[Dict]:
    """The named paths of section "GEMM" (every case runs in both dtypes).  ``expect`` is what stage_ref.gemm_plan must
    say for ``num_cus``; the GPU test asserts it for the device it runs on."""
    full = math.ceil(0.8 * num_cus)
    m_stream = max(4 * num_cus * 256 // 2 + 256, (32 << 20) // (512 * 2)) + 256 + 40
    p_4352 = math.ceil(0.8 * num_cus / 17)
    return [
        dict(name="persist_auto_ragged", M=256 * full + 88, N=256, K=64,
             expect=dict(kernel="gemm256p", stream_out=False, fgroup_active=False)),
        dict(name="persist_multi_tile_stream_out", M=m_stream, N=512, K=64,
             expect=dict(kernel="gemm256p", stream_out=True, fgroup_active=False), min_tiles_per_wg=5),
        dict(name="persist_fgroup", M=13 * 256 + 72, N=4096, K=1024,
             expect=dict(kernel="gemm256p", stream_out=False, fgroup_active=True)),
        dict(name="gemm256_auto", M=256 * max(p_4352 - 1, 0) + 40, N=4352, K=64,
             expect=dict(kernel="gemm256", stream_out=False, fgroup_active=False)),
    ]


def gemm_inputs(seed: int, name: str, dtype: str, M: int, N: int, K: int, device, z_std: float = 1.5,
                ldx: int = 0) -> Dict:
    """Wide operands: X ~ N(0, 1), W ~ N(0, z_std^2 / K) (pre-activations of spread z_std whatever K), bias ~ N(0, 0.5^2):
    a shifted bias column, a dropped K-slab or a neighbour's row moves an output by far more than the bound."""
    ldx = ldx or K
    X = t16(syn.normal(seed, name + ".x", (M, ldx)), dtype, device)
    W = t16(syn.normal(seed, name + ".w", (N, K), std=z_std / math.sqrt(K)), dtype, device)
    b = t32(syn.normal(seed, name + ".b", (N,), std=0.5), device)
    return dict(X=X, W=W, bias=b)


def sweep_values(dtype: str) -> torch.Tensor:
    """Every non-negative value of the 16-bit type up to 6.0, ascending (fp16: 17,921 values; bf16: 16,577)."""
    top = {"f16": 0x4600, "bf16": 0x40C0}[dtype]
    bits = torch.arange(0, top + 1, dtype=torch.int32).to(torch.int16)
    return bits.view(R.TDT[dtype])


def gelu_sweep_inputs(dtype: str, device) -> Dict:
    """K = 64, N = 128.  W[f] = +e_f for f < 64 and -e_(f-64) for f >= 64 (unit vectors), bias 0, X holding every
    non-negative value of the type up to 6 once (the last row padded with 6): the pre-activation z[t, f] = +-X[t, f % 64]
    is EXACT in the kernel (one non-zero product per sum) and takes every value of the type in [-6, 6]."""
    vals = sweep_values(dtype)
    M = (vals.numel() + 63) // 64
    X = torch.full((M * 64,), 6.0, dtype=R.TDT[dtype])
    X[:vals.numel()] = vals
    W = torch.zeros(128, 64, dtype=R.TDT[dtype])
    idx = torch.arange(64)
    W[idx, idx] = 1.0
    W[64 + idx, idx] = -1.0
    return dict(X=X.view(M, 64).to(device), W=W.to(device), bias=torch.zeros(128, dtype=torch.float32, device=device),
                M=M, N=128, K=64)


# ======================================================================================================================
# LayerNorm family
# ======================================================================================================================
def ln_inputs(seed: int, name: str, rows: int, H: int, device, stride_rows: int = 1) -> Dict:
    """A residual stream with mean >> spread and outlier channels (as synthetic.encoder_weights(tail="heavy") gives a
    trained encoder's): x = 8 + N(0, 0.25^2) per element plus a per-row offset N(0, 2^2), six channels 20x wider; the two
    branch outputs fp16 N(0, 0.5^2) (large enough that folding one twice shows); gamma = 1 + N(0, 0.1^2) with six 6x gains,
    beta ~ N(0, 1) (so that many outputs sit near zero, where the store's relative rounding leaves the statistics'
    errors visible).  Row 0 is CONSTANT (0.5, both branch rows zero: variance exactly 0, so only eps keeps rstd finite)
    and row 1 has a spread of 1e-3 around 0 (variance 1e-6: below eps = 1e-5, far above 1e-12) whenever the case has
    three rows or more (a one-row case keeps its row generic: it cannot hold both).  Arrays are [rows * stride_rows, H]; row r of the pass is row r * stride_rows."""
    n = rows * stride_rows
    x = syn.normal(seed, name + ".x", (n, H), std=0.25) + 8.0 + syn.normal(seed, name + ".off", (n, 1), std=2.0)
    ch = np.random.Generator(np.random.Philox(key=[seed, 77])).choice(H, size=6, replace=False)
    x[:, ch] += syn.normal(seed, name + ".out", (n, 6), std=5.0)
    dA = syn.normal(seed, name + ".dA", (n, H), std=0.5)
    dB = syn.normal(seed, name + ".dB", (n, H), std=0.5)
    if rows >= 3:
        x[0], dA[0], dB[0] = 0.5, 0.0, 0.0
        r = stride_rows
        x[r] = syn.normal(seed, name + ".low", (H,), std=1e-3)
        dA[r], dB[r] = 0.0, 0.0
    g = syn.normal(seed, name + ".g", (H,), std=0.1, mean=1.0)
    g[ch] *= 6.0
    b = syn.normal(seed, name + ".b", (H,), std=1.0)
    return dict(x=t32(x, device), dA=t16(dA, "f16", device), dB=t16(dB, "f16", device), gamma=t32(g, device),
                beta=t32(b, device))


def embed_inputs(seed: int, name: str, B: int, T: int, H: int, device) -> Dict:
    """vm_embed operands cut from ln_inputs: fp16 patch rows [B * (T - 1), H], cls [H], pos [T, H] (offset 8, outlier
    channels).  Token 2 of every frame is CONSTANT (pos 0.25 + patch 0.25: variance exactly 0, only eps keeps the
    pre-LayerNorm finite) and token 3 has a spread of 1e-3 around 0 (patch row zero): T >= 4."""
    ins = ln_inputs(seed, name, B * T, H, device)
    patch = ins["dA"][:B * (T - 1)].clone().view(B, T - 1, H)
    pos = ins["x"][:T].clone()
    pos[2], patch[:, 1] = 0.25, 0.25
    pos[3] = t32(syn.normal(seed, name + ".low", (H,), std=1e-3), device)
    patch[:, 2] = 0.0
    return dict(patch16=patch.view(B * (T - 1), H).contiguous(), cls=ins["beta"], pos=pos.contiguous(),
                gamma=ins["gamma"], beta=ins["beta"])


# ======================================================================================================================
# attention
# ======================================================================================================================
def attention_inputs(seed: int, name: str, dtype: str, B: int, T: int, heads: int, device) -> torch.Tensor:
    """qkv head-major [3 * heads][B * T][64].  q, k ~ N(0, 1.5^2): logits q.k / 8 of spread ~2.3 (peaked rows, a handful
    of keys carry a row); v ~ N(0, 1).  In every sequence the LAST valid key is made dominant for the queries of the
    second half (k_last = 3 q-direction): masking it, or a stale K/V image of the previous item, moves those rows by
    O(1); and v of the last key is large (8) so an unmasked neighbour or its loss shows in every channel.

    CONTRACT about the bytes behind the operand: the kernels clamp every key / query row index to T - 1 of its own
    sequence (attention.hip: `if (key > T - 1) key = T - 1`), so nothing beyond the [3 * heads][B * T][64] elements is
    read; the operand is exactly that long, with no tile padding."""
    q = syn.normal(seed, name + ".q", (heads, B, T, 64), std=1.5)
    k = syn.normal(seed, name + ".k", (heads, B, T, 64), std=1.5)
    v = syn.normal(seed, name + ".v", (heads, B, T, 64), std=1.0)
    d = syn.normal(seed, name + ".dir", (heads, B, 1, 64), std=1.0)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    half = T // 2
    q[:, :, half:, :] += 4.0 * d                    # the later queries share a direction ...
    k[:, :, T - 1, :] = 6.0 * d[:, :, 0, :]        # ... that the last key answers: logit ~ +3 over the rest
    v[:, :, T - 1, :] = 8.0
    qkv = np.concatenate([q, k, v], axis=0).reshape(3 * heads, B * T, 64)
    return t16(qkv, dtype, device)


# T -> the arm stage_ref.attention_plan must name, and the heads counts run at that T (1, 4, 12 and 16 all appear)
ATTENTION_ARMS = {
    1: ("plain2", (1, 4)), 16: ("plain2", (12,)), 17: ("plain2", (16,)), 32: ("plain2", (4,)),
    33: ("plain5", (1, 12)), 80: ("plain5", (16,)),
    81: ("plain13", (4,)), 197: ("stream13", (12,)), 208: ("stream13", (1, 16)),
    209: ("long37_persist_few", (4,)), 226: ("long37_pair12", (12,)),
    577: ("long37_exact_persist_few", (16,)), 592: ("long37_exact_persist_few", (1,)),
}
ATTENTION_Q1_ARMS = {"plain2": "plain2", "plain5": "plain5", "plain13": "plain13", "stream13": "stream13",
           "long37_persist_few": "long37_persist_many", "long37_pair12": "long37_persist_many",
           "long37_exact_persist_few": "long37_exact_persist_many"}


def split_qkv(qkv: torch.Tensor, B: int, T: int, heads: int):
    """[3 * heads][B * T][64] -> q, k, v as [B * heads, T, 64] with group index b * heads + head."""
    x = qkv.view(3, heads, B, T, 64).permute(0, 2, 1, 3, 4).reshape(3, B * heads, T, 64)
    return x[0], x[1], x[2]


# ======================================================================================================================
# record of the measured headroom (profiles/stage_parity.json is one GPU run's copy of it)
# ======================================================================================================================
RECORD: Dict[str, Dict[str, float]] = {}


def record(family: str, case: str, ratio: float) -> None:
    """Keep the worst error / bound ratio seen per case."""
    fam = RECORD.setdefault(family, {})
    fam[case] = max(fam.get(case, 0.0), float(ratio))


def flush_record(family: str, seconds: float) -> None:
    """Merge this family's ratios and run time into the JSON file named by STAGE_PARITY_JSON (unset: nothing is written;
    the tests assert, the file only reports)."""
    import json
    import os
    path = os.environ.get("STAGE_PARITY_JSON")
    if not path:
        return
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc["device"] = torch.cuda.get_device_name(0) if torch.cuda.is_available() else "cpu"
    doc.setdefault("families", {})[family] = dict(
        seconds=round(seconds, 2), worst_ratio=max(RECORD.get(family, {"": 0.0}).values()),
        cases={k: float(f"{v:.4g}") for k, v in sorted(RECORD.get(family, {}).items())})
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
