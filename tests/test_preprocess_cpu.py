"""CPU: the model and the case table of tests/preprocess_ref.py, which tests/test_preprocess_gpu.py holds vm_preprocess to.

* the oracle (oracle/frames_ref.py preprocess_ref) equals the per-element restatement of include/vidmem.h bit for bit on
  the small cases and lies within the derived rounding bound of the float64 evaluation on every case;
* the emulation of the kernel's index and tap arithmetic equals the oracle's bits on every case, so a planted defect is
  the only thing that separates them;
* the table holds what the GPU comparison needs in order not to pass vacuously: ties, f16 subnormals, exact +0.0, clamped
  taps on all four sides, pad regions of several widths, every kernel instance, the fast path and its neighbours;
* every planted defect changes the output bits of the cases named in SEEN_BY (and of at least one case at all).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import preprocess_ref as P
from tests.support import TD

SMALL = [c.name for c in P.CASES if P.is_small(c)]
MEDIUM = [c for c in P.CASES if P.n_out(c) <= 40000]  # what the defects are planted in: every branch, a few ms each


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_bits16_is_the_ieee_cast(dtype):
    """bits16 against torch's cast on ties, subnormals, signed zeros and a case's whole output."""
    rng = np.random.default_rng(3)
    special = np.array([0.0, -0.0, 2.0 ** -14, 2.0 ** -15, -2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 1 + 2.0 ** -11,
                        1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -8), 1 + 3 * 2.0 ** -8, 2.0 ** -14 - 2.0 ** -25, 65504.0, -2.6],
                       np.float32)
    x = np.concatenate([special, rng.standard_normal(4096).astype(np.float32) * np.float32(2.0 ** -13),
                        P.oracle_cached("generic-p8-k192-f16")])
    want = torch.from_numpy(x).to(TD[dtype]).view(torch.int16).numpy()
    assert np.array_equal(P.bits16(x, dtype), want)
    # the two wrong casts differ from it where they must, and nowhere else
    rtz, away = P.bits16(x, dtype, "rtz"), P.bits16(x, dtype, "half_away")
    back = torch.from_numpy(want).view(TD[dtype]).float().numpy()
    assert np.array_equal(rtz != want, np.abs(back) > np.abs(x))
    assert ((away != want) <= (back != x)).all() and (away != want).any()


@pytest.mark.parametrize("name", SMALL)
def test_oracle_equals_scalar_model(name):
    case = P.BY_NAME[name]
    got, want = P.oracle_cached(name), P.scalar_model(case)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), \
        f"{name}: {(got.view(np.int32) != want.view(np.int32)).sum()} fp32 bit patterns differ"


@pytest.mark.parametrize("name", [c.name for c in P.CASES])
def test_oracle_within_rounding_bound_of_fp64(name):
    case = P.BY_NAME[name]
    exact, bound = P.exact_fp64(case)
    err = np.abs(P.oracle_cached(name).astype(np.float64) - exact)
    assert (bound[~P.pad_mask(case)] > 0).all() and (err <= bound).all(), \
        f"{name}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}"


@pytest.mark.parametrize("name", [c.name for c in P.CASES])
def test_emulation_equals_oracle(name):
    case = P.BY_NAME[name]
    assert np.array_equal(P.emulate(case), P.bits16(P.oracle_cached(name), case.dtype))


def test_table_conditions():
    """What the bit comparison on the GPU needs to meet, per dtype, counted in the oracle's output."""
    for dtype in ("f16", "bf16"):
        rows = [P.census(c) for c in P.CASES if c.dtype == dtype]
        total = {k: sum(r[k] for r in rows) for k in rows[0]}
        print(dtype, total)
        assert total["ties"] >= 100, (dtype, total)
        assert total["f16_subnormal"] >= 20, (dtype, total)
        assert total["plus_zero"] >= 100, (dtype, total)
        for side in ("clamp_top", "clamp_bottom", "clamp_left", "clamp_right"):
            assert total[side] > 0, (dtype, side)
        widths = {r["pad_columns"] for r in rows} - {0}
        assert len(widths) >= 2, (dtype, widths)
        assert any(r["clamp_top"] >= 8 and r["clamp_left"] >= 8 for r in rows), "no large upscale"


def test_table_covers_every_branch():
    def instance(c):
        if c.layout == "chw":
            return "chw"
        return {(16, 768): "<16,768>", (14, 640): "<14,640>"}.get((c.patch, c.k_pad), "<0,0>")

    have = {(c.dtype, instance(c)) for c in P.CASES}
    assert have == {(d, i) for d in ("f16", "bf16") for i in ("chw", "<16,768>", "<14,640>", "<0,0>")}
    for dtype in ("f16", "bf16"):
        cs = [c for c in P.CASES if c.dtype == dtype]
        assert {c.S for c in cs if P.is_fast(c)} >= {32, 64, 224}
        near = [c for c in cs if c.patch == 16 and c.k_pad == 768 and not P.is_fast(c, aligned=True)]
        assert any(c.H == c.S and c.W != c.S for c in near) and any(c.W == c.S and c.H != c.S for c in near)
        assert any((c.H, c.W) == (1, 1) for c in cs) and any(c.H == 1 and c.W > 1 for c in cs)
        assert any(c.W == 1 and c.H > 1 for c in cs)
        assert any(c.B is P.WRAP for c in cs)
        assert any(c.B and c.B > 1 and (c.H * c.W * 3) % 8 for c in cs)
    # misaligned frame pointers at sizes the fast path would otherwise serve, and on the general path
    off = [c for c in P.CASES if c.offset % 8]
    assert {c.offset for c in off if P.is_fast(c, aligned=True)} >= {1, 3, 5}
    assert any(not P.is_fast(c, aligned=True) for c in off)
    assert {c.dtype for c in off if P.is_fast(c, aligned=True)} == {"f16", "bf16"}
    # run-time divisors with pad regions of 0, 4 and more columns
    gen = [c for c in P.CASES if instance(c) == "<0,0>"]
    assert {c.k_pad - 3 * c.patch ** 2 for c in gen} >= {0, 4, 8, 64} and {c.patch for c in gen} >= {8, 14, 32}
    assert all(c.S % 8 == 0 and (c.layout == "chw" or (c.S % c.patch == 0 and c.k_pad % 8 == 0)) for c in P.CASES)


# cases that must see a defect, from what the defect touches (the test prints the whole map)
SEEN_BY = {
    "bgr_not_swapped": ("fast-f16-32", "generic-p8-k192-bf16", "thin-f16-1x1-chw"),
    "align_corners": ("ratio2-f16-random", "corners-bf16-up"),
    "no_low_clamp": ("corners-f16-up", "thin-f16-1x1-chw"),
    "lam_before_clamp": ("corners-f16-up", "thin-f16-1x9-chw"),
    "scales_swapped": ("thin-f16-1x9-chw", "ratio3x1-f16-random"),
    "frame_stride": ("generic-p8-k192-f16", "wrap-f16-40x56"),
    "pyx_c_order": ("fast-f16-32", "generic-p32-k3072-f16"),
    "pad_nonzero": ("generic-p14-k592-f16", "generic-p16-k776-f16", "p14-f16-97x131", "generic-p8-k256-bf16"),
    "pad_threshold": ("generic-p14-k592-f16", "generic-p16-k776-f16", "p14-f16-97x131", "generic-p8-k256-bf16"),
    "fused_affine": ("generic-p8-k192-f16", "generic-p8-k192-bf16"),
    "cast_rtz": ("fast-f16-32", "fast-bf16-32"),
    "cast_half_away": ("generic-p8-k192-f16", "generic-p8-k192-bf16"),
    "flush_subnormal": ("generic-p14-k592-f16", "generic-p8-k192-bf16"),
    "minus_zero": ("rows127-f16-2to1", "rows127-bf16-2to1"),
    "fast_when_h_only": ("near-f16-64x65", "near-bf16-64x128"),
    "fast_e7_pixel6": ("fast-f16-32", "fast-bf16-64"),
}
# ... and cases that must not: the defect's branch or operand is not theirs
NOT_SEEN_BY = {
    "fast_when_h_only": ("near-f16-63x64", "fast-f16-64"),
    "fast_e7_pixel6": ("offset1-fast-f16-64", "near-f16-64x65"),
    "lam_before_clamp": ("thin-f16-1x1-chw", "fast-f16-32"),
    "scales_swapped": ("ratio2-f16-random",),
    "pad_nonzero": ("generic-p8-k192-f16",),
}


@pytest.fixture(scope="module")
def sound():
    return {c.name: P.emulate(c) for c in MEDIUM}


@pytest.mark.parametrize("defect", P.DEFECTS)
def test_every_planted_defect_changes_bits(defect, sound):
    assert set(SEEN_BY) == set(P.DEFECTS)
    seen = [c.name for c in MEDIUM if not np.array_equal(P.emulate(c, defect=defect), sound[c.name])]
    print(f"{defect}: seen by {len(seen)} of {len(MEDIUM)} cases: {seen}")
    assert seen, f"{defect} changes no bit of any case"
    assert set(SEEN_BY[defect]) <= set(seen), sorted(set(SEEN_BY[defect]) - set(seen))
    assert not set(NOT_SEEN_BY.get(defect, ())) & set(seen)
