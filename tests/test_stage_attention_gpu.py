"""GPU: vm_attention alone, every dispatch arm, element by element against fp64 softmax(Q K^T / 8) V
(tests/stage_ref.py), through the test shim (tests/stage_lib.py).

CONTRACT stated and tested here:
  * the operand is exactly [3 * heads][B * T][64] elements: the kernels clamp every row index to T - 1 of its own
    sequence, so there are no bytes between the B * T rows and the end of the last key tile that they may read.  The
    operand is a WINDOW of exactly that length inside one larger 16-bit allocation filled with 0x7FFF - a NaN in fp16
    and in bf16 - with 512 rows of 64 (32 key tiles) in front of the first q block and behind the last v block.  A key
    or value row read past the operand, even against a probability of 0, gives 0 * NaN = NaN in the context, and the
    all-elements-inside-the-bound assertion counts a NaN as outside; the read itself stays inside the allocation;
  * ctx_out rows >= q_rows rounded up to 16 of every sequence are left untouched, as is everything outside [B * T, H].
Inputs have peaked rows and a dominant last key (stage_cases.attention_inputs): a wrong mask, the loss of the last
valid key or a stale K/V image of the previous item moves outputs by O(1), thousands of bounds.
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

ARMS, Q1_ARMS = CS.ATTENTION_ARMS, CS.ATTENTION_Q1_ARMS


@pytest.fixture(scope="module")
def st():
    t0 = time.time()
    s = Stages(0)
    yield s
    CS.flush_record("attention", time.time() - t0)


def run_attention(st, dtype, B, T, heads, q_rows=0, causal=0, seed=200):
    H = heads * 64
    vals = CS.attention_inputs(seed + T, f"attn.{dtype}.{B}.{T}.{heads}", dtype, B, T, heads, DEV)
    rows = 3 * heads * B * T                            # exactly as long as the contract says: no tile padding
    qbuf = torch.full((G + rows + G, 64), CS.NAN16, dtype=torch.int16, device=DEV)
    qkv = qbuf[G:G + rows].view(R.TDT[dtype]).view(3 * heads, B * T, 64)
    qkv.copy_(vals)
    assert bool(torch.isnan(qbuf[:G].view(R.TDT[dtype])).all()) and bool(torch.isnan(qbuf[G + rows:].view(R.TDT[dtype])).all())
    plan = R.attention_plan(T, B, heads, st.num_cus, q_rows=q_rows, causal=causal)
    buf = CS.canary16(G + B * T + G, H, DEV)
    win = buf[G:G + B * T]
    st.ctx.profile_enable(8)
    st.ctx.profile_read()
    st.attention(dtype, qkv, win, B, T, heads, q_rows=q_rows, causal=causal)
    launches = st.ctx.profile_read()["attention"][1]
    st.ctx.profile_enable(0)
    assert launches == 1
    Tq = min(16 * plan["ql"], T)
    wv = win.view(B, T, H)
    got = wv[:, :Tq, :].clone().view(R.TDT[dtype]).float()                    # [B, Tq, H]
    wv[:, :Tq, :].fill_(CS.CANARY16)
    assert CS.untouched(buf), "vm_attention wrote outside the query rows it was asked for"
    q, k, v = CS.split_qkv(qkv, B, T, heads)
    c, bound = R.attention_ref_and_bound(dtype, q[:, :Tq], k, v, bool(causal), plan["NT"])
    if T <= 33:   # the small shapes run the fp64 reference on the CPU once as well
        c_cpu, b_cpu = R.attention_ref_and_bound(dtype, q[:, :Tq].cpu(), k.cpu(), v.cpu(), bool(causal), plan["NT"])
        # same fp64 formula, another summation order: 2^-53 per operation where the bound charges >= U32 = 2^-24 for the
        # kernel's, i.e. 2^-29 of the bound; 2^-20 of it is asserted
        assert bool(((c.cpu() - c_cpu).abs() <= 2.0 ** -20 * b_cpu).all()), "device and CPU fp64 references disagree"
        assert bool(((bound.cpu() - b_cpu).abs() <= 2.0 ** -20 * b_cpu).all()), "device and CPU bounds disagree"
    c = c.view(B, heads, Tq, 64).permute(0, 2, 1, 3).reshape(B, Tq, H)
    bound = bound.view(B, heads, Tq, 64).permute(0, 2, 1, 3).reshape(B, Tq, H)
    ratio, outside = R.worst_ratio(got, c, bound)
    name = f"{dtype}.T{T}.B{B}.h{heads}.q{q_rows}.c{causal}.{plan['arm']}"
    print(f"{name}: worst error / bound = {ratio:.4f}")
    CS.record("attention", name, ratio)
    assert outside == 0, f"{name}: {outside} of {c.numel()} elements outside the bound (worst ratio {ratio:.3f})"
    return plan


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", sorted(ARMS))
def test_attention_arms(st, dtype, T):
    """Every arm of attention.hip's dispatch at its edges (nt <= 2, <= 5, <= 13 inexact, == 13 streaming, <= 37 inexact
    with the persistent and the plain pair walk, == 37), all query rows and q_rows = 1, three sequences each."""
    arm, heads_list = ARMS[T]
    for heads in heads_list:
        assert run_attention(st, dtype, 3, T, heads)["arm"] == arm
        assert run_attention(st, dtype, 3, T, heads, q_rows=1)["arm"] == Q1_ARMS[arm]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,heads", ((197, 12), (577, 16)))
def test_attention_persistent_items(st, dtype, T, heads):
    """B * heads below and above the CU count: above it the persistent kernels (streaming 13-tile, long 37-tile) give
    some workgroups a second item, whose K/V image replaces the first one's."""
    below = max(st.num_cus // heads - 1, 1)
    above = st.num_cus // heads + 1
    assert below * heads < st.num_cus < above * heads
    p = run_attention(st, dtype, below, T, heads)
    assert p["grid"] == below * heads
    p = run_attention(st, dtype, above, T, heads)
    assert p["grid"] == st.num_cus


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", (1, 16, 17, 77, 80))
def test_attention_causal(st, dtype, T):
    """The text tower's mask: key j > query i is masked; one 5-tile build for every T <= 80."""
    for heads in ((1, 12) if T == 77 else (4,) if T < 17 else (16,)):
        assert run_attention(st, dtype, 3, T, heads, causal=1)["arm"] == "causal5"
