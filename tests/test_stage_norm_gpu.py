"""GPU: the LayerNorm / embed / pool / text-embed kernels of csrc/encoder.hip alone, element by element against fp64
(tests/stage_ref.py), through the test shim (tests/stage_lib.py).

Every output lives in a window of a larger canary-filled allocation (512 guard rows on both sides); the guards and every
row the launcher's contract leaves alone (rows between the strided ones, x32 rows `write_x` does not select) must keep
their bits.  Where a result is fully determined - the x32 write-back (two fp32 additions), embed without pre-LN, the
whole of vm_text_embed - the tests assert bit equality, not a bound.
"""
import itertools
import time

import pytest
import torch

import tests.stage_cases as CS
import tests.stage_ref as R
from tests.stage_lib import Stages

pytestmark = pytest.mark.gpu

DTYPES = ("f16", "bf16")
HS = (256, 512, 768, 1024)
G = CS.GUARD_ROWS
DEV = "cuda"
T_FRAME = 197


@pytest.fixture(scope="module")
def st():
    t0 = time.time()
    s = Stages(0)
    yield s
    CS.flush_record("norm", time.time() - t0)


def check(case, got, y, bound):
    ratio, outside = R.worst_ratio(got, y, bound)
    CS.record("norm", case, ratio)
    assert outside == 0, f"{case}: {outside} of {y.numel()} elements outside the bound (worst ratio {ratio:.3f})"
    return ratio


def same_on_cpu(y, bound, cpu_pair):
    """The small shapes run the fp64 reference on the CPU once as well: device and CPU must agree far inside the bound.
    Both evaluate the same fp64 formula with sums over at most H = 1024 terms in different orders: the results differ by
    rounding of 2^-53 per operation, amplified like the kernel's own fp32 roundings that `bound` is made of - so
    2^-53 / U32 = 2^-29 of the bound covers any order; 2^-20 of it is asserted (512 times that)."""
    y_cpu, bound_cpu = cpu_pair
    assert bool(((y.cpu() - y_cpu).abs() <= 2.0 ** -20 * bound_cpu).all()), "device and CPU fp64 references disagree"
    assert bool(((bound.cpu() - bound_cpu).abs() <= 2.0 ** -20 * bound_cpu).all()), "device and CPU bounds disagree"


def run_ln(st, dtype, ins, rows, H, rstride, write_x, use_a, use_b, eps, lowreg):
    """One vm_resid_layernorm launch on canary-windowed copies; returns (out16 rows as int16 [rows, H], x32 after [n, H])
    after asserting the guards, the rows between the strided ones and the unselected x32 rows."""
    n = rows * rstride
    xbuf = CS.canary32(G + n + G, H, DEV)
    xwin = xbuf[G:G + n]
    xwin.view(torch.float32).copy_(ins["x"])
    obuf = CS.canary16(G + n + G, H, DEV)
    owin = obuf[G:G + n]
    st.resid_layernorm(dtype, xwin, ins["dA"] if use_a else None, ins["dB"] if use_b else None, write_x, ins["gamma"],
                       ins["beta"], eps, owin, rows, H, rstride=rstride, lowreg=lowreg)
    torch.cuda.synchronize()
    out = owin[::rstride].clone()
    owin[::rstride].fill_(CS.CANARY16)
    assert CS.untouched(obuf), "vm_resid_layernorm wrote out16 outside its rows"
    xafter = xwin.clone()
    xwin.fill_(CS.CANARY32)
    assert CS.untouched(xbuf), "vm_resid_layernorm wrote x32 outside its rows"
    return out, xafter.view(torch.float32)


def ln_sweep(st, dtype, H, rows_list, tag):
    worst = 0.0
    for rows in rows_list:
        big = rows > 9
        for rstride in (1, 4 if big else T_FRAME):
            ins = CS.ln_inputs(70 + H // 256, f"ln.{H}.{rows}.{rstride}", rows, H, DEV, stride_rows=rstride)
            v32 = R.resid_sum32  # the fp32 restatement of the row the kernel normalises and may write back
            for use_a, use_b, eps in itertools.product((0, 1), (0, 1), (1e-12, 1e-5)):
                xs = ins["x"][::rstride]
                dA = ins["dA"][::rstride] if use_a else None
                dB = ins["dB"][::rstride] if use_b else None
                y, bound = R.resid_layernorm_ref_and_bound(dtype, xs, dA, dB, ins["gamma"], ins["beta"], eps)
                if not big:
                    same_on_cpu(y, bound, R.resid_layernorm_ref_and_bound(
                        dtype, xs.cpu(), None if dA is None else dA.cpu(), None if dB is None else dB.cpu(),
                        ins["gamma"].cpu(), ins["beta"].cpu(), eps))
                vexp = v32(xs, dA, dB)
                ref_out = None
                for write_x, lowreg in itertools.product((0, 1, T_FRAME if big else 4), (0, 1)):
                    assert R.ln_plan(rows, H, lowreg) == ("lowreg_nt" if lowreg else tag)
                    out, xafter = run_ln(st, dtype, ins, rows, H, rstride, write_x, use_a, use_b, eps, lowreg)
                    r = check(f"{dtype}.ln.H{H}.rows{rows}", out.view(R.TDT[dtype]).float(), y, bound)
                    worst = max(worst, r)
                    # the two builds (and every write_x) must agree bit for bit: the two-stream schedule relies on it
                    if ref_out is None:
                        ref_out = out
                    assert torch.equal(out, ref_out), "LayerNorm builds / write_x settings disagree in out16 bits"
                    # x32: selected rows hold the two fp32 additions exactly, every other row its old bits
                    want = ins["x"].clone()
                    if write_x:
                        selr = torch.arange(rows, device=DEV)
                        selr = selr[selr % write_x == 0] if write_x > 1 else selr
                        want[selr * rstride] = vexp[selr]
                    assert torch.equal(xafter.view(torch.int32), want.view(torch.int32)), \
                        f"x32 after the pass (write_x={write_x}, lowreg={lowreg}) is not the fp32 restatement"
    print(f"{dtype} H={H} rows={rows_list}: worst error / bound = {worst:.4f}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", HS)
def test_resid_layernorm(st, dtype, H):
    """rows in {1, 7, 8, 9, 3 * 197} (one wave, a partial / exact / one-past block of the two-rows-per-wave build, several
    blocks) x write_x in {0, 1, T} x every null / non-null combination of the two branch outputs x rstride in {1, T} x
    both builds x eps in {1e-12, 1e-5}."""
    ln_sweep(st, dtype, H, (1, 7, 8, 9, 3 * T_FRAME), "plain")


@pytest.mark.parametrize("dtype", DTYPES)
def test_resid_layernorm_non_temporal(st, dtype):
    """rows * H * 4 > 64 MiB: the non-temporal build of the ordinary kernel (H = 1024, 16,392 rows) beside the
    low-register build (always non-temporal); one setting of the other switches."""
    H, rows = 1024, 16392
    assert R.ln_plan(rows, H, 0) == "plain_nt" and R.ln_plan(rows - 8, H, 0) == "plain"
    ins = CS.ln_inputs(90, "ln.nt", rows, H, DEV)
    y, bound = R.resid_layernorm_ref_and_bound(dtype, ins["x"], ins["dA"], ins["dB"], ins["gamma"], ins["beta"], 1e-5)
    vexp = R.resid_sum32(ins["x"], ins["dA"], ins["dB"])
    outs = []
    for lowreg in (0, 1):
        st.ctx.profile_enable(8)
        st.ctx.profile_read()
        out, xafter = run_ln(st, dtype, ins, rows, H, 1, 1, 1, 1, 1e-5, lowreg)
        launches = st.ctx.profile_read()["layernorm"][1]
        st.ctx.profile_enable(0)
        assert launches == 1, "vm_resid_layernorm is one kernel launch in the layernorm category"
        check(f"{dtype}.ln.nt.lowreg{lowreg}", out.view(R.TDT[dtype]).float(), y, bound)
        assert torch.equal(xafter.view(torch.int32), vexp.view(torch.int32))
        outs.append(out)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", HS)
def test_embed(st, dtype, H):
    """vm_embed with and without the pre-LayerNorm, T in {5, 197}, eps in {1e-12, 1e-5}.  Without pre-LN the result is
    one fp32 addition per element: bit equality.  With it: fp32 out, the LayerNorm bound without a store term."""
    for (B, T), eps in itertools.product(((3, 5), (2, T_FRAME)), (1e-12, 1e-5)):
        ins = CS.embed_inputs(100 + T, f"embed.{H}.{T}", B, T, H, DEV)
        patch16, cls, pos = ins["patch16"], ins["cls"], ins["pos"]   # fp16 patch rows whatever the dtype (EPI_DELTA16)
        for pre_ln in (0, 1):
            buf = CS.canary32(G + B * T + G, H, DEV)
            win = buf[G:G + B * T]
            st.ctx.profile_enable(8)
            st.ctx.profile_read()
            st.embed(dtype, patch16, cls, pos, ins["gamma"], ins["beta"], eps, pre_ln, win, B, T, H)
            assert st.ctx.profile_read()["layernorm"][1] == 1    # vm_embed's category (encoder.hip)
            st.ctx.profile_enable(0)
            got = win.view(torch.float32).clone().view(B, T, H)
            win.fill_(CS.CANARY32)
            assert CS.untouched(buf), "vm_embed wrote outside its B * T rows"
            if not pre_ln:
                want = R.embed_exact32(patch16, cls, pos, B, T)
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "embed without pre-LN is not exact"
            else:
                y, bound = R.embed_ref_and_bound(patch16, cls, pos, ins["gamma"], ins["beta"], eps, True, B, T)
                check(f"{dtype}.embed.H{H}.T{T}.pre_ln", got, y, bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", HS)
def test_pool(st, dtype, H):
    """vm_pool: proj_dim in {0, 128, 768} x l2 in {0, 1} x with / without pool_row, eps in {1e-12, 1e-5}."""
    B, T = 4, 7
    ins = CS.ln_inputs(120, f"pool.{H}", B * T, H, DEV)
    prow = torch.tensor([0, 6, 3, 1], dtype=torch.int32, device=DEV)
    for proj_dim, l2, with_row, eps in itertools.product((0, 128, 768), (0, 1), (0, 1), (1e-12, 1e-5)):
        od = proj_dim or H
        pw = CS.t16(CS.syn.normal(121, f"pool.w.{proj_dim}.{H}", (max(proj_dim, 1), H), std=0.05), dtype, DEV)
        buf = CS.canary16(G + B + G, od, DEV)
        win = buf[G:G + B]
        st.ctx.profile_enable(8)
        st.ctx.profile_read()
        st.pool(dtype, ins["x"], ins["dA"], ins["dB"], ins["gamma"], ins["beta"], eps, pw if proj_dim else None,
                proj_dim, l2, win, B, T, H, pool_row=prow if with_row else None)
        assert st.ctx.profile_read()["pool"][1] == 1
        st.ctx.profile_enable(0)
        got = win.clone().view(R.TDT[dtype]).float()
        win.fill_(CS.CANARY16)
        assert CS.untouched(buf), "vm_pool wrote outside its B rows"
        rows = torch.arange(B, device=DEV) * T + (prow.long() if with_row else 0)
        y, bound = R.pool_ref_and_bound(dtype, ins["x"][rows], ins["dA"][rows], ins["dB"][rows], ins["gamma"],
                                        ins["beta"], eps, pw if proj_dim else None, bool(l2))
        check(f"{dtype}.pool.H{H}.proj{proj_dim}.l2_{l2}.row{with_row}", got, y, bound)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_zero_row_under_l2(st, dtype):
    """CONTRACT: with l2 = 1 the norm is clamped at 1e-12 (pool_kernel: 1 / fmaxf(nrm, 1e-12)), so an all-zero pooled
    vector comes out as zeros, never NaN or inf.  gamma = beta = 0 makes every LayerNorm output exactly 0."""
    B, T, H = 3, 5, 512
    ins = CS.ln_inputs(130, "pool.zero", B * T, H, DEV)
    zero = torch.zeros(H, dtype=torch.float32, device=DEV)
    for proj_dim in (0, 128):
        od = proj_dim or H
        pw = CS.t16(CS.syn.normal(131, "pool.zero.w", (128, H), std=0.05), dtype, DEV)
        buf = CS.canary16(G + B + G, od, DEV)
        win = buf[G:G + B]
        st.pool(dtype, ins["x"], ins["dA"], ins["dB"], zero, zero, 1e-5, pw if proj_dim else None, proj_dim, 1, win, B, T, H)
        torch.cuda.synchronize()
        got = win.clone().view(R.TDT[dtype]).float()
        assert bool((got == 0).all()), "a zero row under l2 = 1 is not all zeros"


def test_text_embed(st):
    """vm_text_embed is fully determined: x32 bit for bit, pool_row and flags exactly.  ids below 0 and >= vocab (clamped,
    flag bit 0), no EOT (flag bit 1, pool_row 0), EOT at 0 and at T - 1, two EOTs (the first wins), T beyond one 64-lane
    scan step."""
    vocab, eot = 1000, 999
    for H, T in itertools.product(HS, (5, 77, 130)):
        B = 7
        g = torch.Generator().manual_seed(140 + T)
        ids = torch.randint(0, vocab - 1, (B, T), generator=g, dtype=torch.int32)
        ids[0, 0] = eot                                   # EOT at 0
        ids[1, T - 1] = eot                               # EOT at T - 1
        ids[2, 2], ids[2, 4] = eot, eot                   # two: the first wins
        ids[3, 1], ids[3, 3] = -5, vocab + 7              # clamped, and no EOT
        ids[4, 1], ids[4, T - 2] = vocab, eot             # clamped, with EOT
        ids[5, T // 2] = eot                              # plain
        ids = ids.to(DEV)                                 # row 6: no EOT, nothing clamped
        tok = CS.t32(CS.syn.normal(141, f"text.tok.{H}", (vocab, H), std=1.0), DEV)
        pos = CS.t32(CS.syn.normal(142, f"text.pos.{H}", (T, H), std=1.0), DEV)
        buf = CS.canary32(G + B * T + G, H, DEV)
        win = buf[G:G + B * T]
        meta = CS.canary32(2, G + B + G, DEV)              # pool_row and flags: B values between 512 guard elements each
        prow, flags = meta[0, G:G + B], meta[1, G:G + B]
        st.ctx.profile_enable(8)
        st.ctx.profile_read()
        st.text_embed(ids, tok, pos, vocab, eot, win, prow, flags, B, T, H)
        assert st.ctx.profile_read()["layernorm"][1] == 1    # the embedding stage's category (encoder.hip)
        st.ctx.profile_enable(0)
        want_x, want_row, want_flags = R.text_embed_exact(ids, tok, pos, vocab, eot)
        assert torch.equal(win.view(B, T, H), want_x.view(torch.int32)), "text embedding rows are not exact"
        assert torch.equal(prow, want_row) and torch.equal(flags, want_flags)
        assert want_flags.tolist() == [0, 0, 0, 3, 1, 0, 2] and want_row.tolist() == [0, T - 1, 2, 0, T - 2, T // 2, 0]
        win.fill_(CS.CANARY32)
        prow.fill_(CS.CANARY32)
        flags.fill_(CS.CANARY32)
        assert CS.untouched(buf) and CS.untouched(meta), "vm_text_embed wrote outside its outputs"
        # flags may be null
        st.text_embed(ids, tok, pos, vocab, eot, buf[G:G + B * T], prow, None, B, T, H)
        torch.cuda.synchronize()
        assert torch.equal(prow, want_row)
        prow.fill_(CS.CANARY32)
        assert CS.untouched(meta), "vm_text_embed with null flags wrote outside pool_row"
