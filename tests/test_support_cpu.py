"""CPU: the shared checker of tests/support.py catches what it must, and ``to_bits`` rounds as the rounding done by hand.

``check_entries`` is driven with closures over CPU tensors: a hand-made answer of Q = 3, k = 4 with -1 padding, a +0.0
score and an int32 third output.  The faithful answer passes; every planted defect raises, planted in the fast entry only
and in the exact entry only.  ``redone`` is driven the same way.
"""
import numpy as np
import pytest
import torch

from tests.support import check_entries, redone, to_bits

Q, K = 3, 4
WANT = (np.array([[5, 2, 9, -1], [7, -1, -1, -1], [1, 3, 4, 6]], dtype=np.int64),
        np.array([[0.9, 0.5, 0.0, 0.0], [0.25, 0.0, 0.0, 0.0], [1.0, 0.75, -0.125, -0.5]], dtype=np.float64),
        np.array([[0, 1, 2, -1], [1, -1, -1, -1], [2, 2, 0, 1]], dtype=np.int32))
ENTRIES = ["fast", "exact"]


def _faithful():
    return [w.copy() for w in WANT]


def _run(fast=None, exact=None, flags=(0, 0, 0), certified=None, label="case"):
    """check_entries over two answers (default: the faithful one), as tensors, and the given fast-entry flags."""
    answers = {False: fast or _faithful(), True: exact or _faithful()}
    return check_entries(lambda e: tuple(torch.from_numpy(a) for a in answers[e]),
                         lambda: torch.tensor(flags, dtype=torch.int32), WANT, certified, label)


# ---- the planted answers: name -> (output it is planted in, function that spoils a faithful answer in place) -------------
def _row_changed(a):
    a[0][2, 1] = 8


def _last_mantissa_bit(a):
    a[1].view(np.int64)[0, 0] ^= 1


def _negative_zero(a):
    assert a[1][0, 2] == 0.0 and not np.signbit(a[1][0, 2]) and a[0][0, 2] == 9      # a real hit whose score is +0.0
    a[1][0, 2] = -0.0


def _third_as_int64(a):
    a[2] = a[2].astype(np.int64)


def _one_column_more(a):
    a[0] = np.concatenate([a[0], np.full((Q, 1), -1, np.int64)], axis=1)


def _row_in_the_padding(a):
    assert a[0][1, 1] == -1
    a[0][1, 1] = 3


PLANTS = {"row": ("rows", _row_changed), "mantissa": ("scores", _last_mantissa_bit), "minus_zero": ("scores", _negative_zero),
          "int64": ("output 2", _third_as_int64), "shape": ("rows", _one_column_more), "padding": ("rows", _row_in_the_padding)}


def test_faithful_answer_passes_and_returns_the_fast_entry():
    fast = _faithful()
    got = _run(fast=fast, flags=(0, 1, 3))
    assert len(got) == 4
    for g, w in zip(got[:3], WANT):
        assert isinstance(g, np.ndarray) and g.dtype == w.dtype and np.array_equal(g, w)
    assert got[3].tolist() == [0, 1, 3]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("plant", list(PLANTS))
def test_planted_answer_raises(plant, entry):
    output, spoil = PLANTS[plant]
    bad = _faithful()
    spoil(bad)
    with pytest.raises(AssertionError) as err:
        _run(label="planted", **{entry: bad})
    text = str(err.value)
    assert "planted" in text and f"{output} of the {entry} entry" in text, text
    other = "exact" if entry == "fast" else "fast"
    assert f"the {other} entry" not in text, text
    if plant in ("row", "padding"):
        assert "got 8, want 3" in text or "got 3, want -1" in text, text             # position and both values
    if plant == "minus_zero":
        assert "got -0.0" in text and "want 0.0" in text and "[0, 2]" in text, text


def test_fast_entry_outputs_are_returned_even_when_the_exact_entry_differs_only():
    """The fast entry's outputs are what the caller goes on to assert about; a defect of the exact entry still raises."""
    bad = _faithful()
    _row_changed(bad)
    with pytest.raises(AssertionError, match="exact entry"):
        _run(exact=bad)


def test_flag_on_a_certified_query_raises():
    for certified in (True, [False, True, False], np.array([True, True, True])):
        with pytest.raises(AssertionError, match="left queries to the redo"):
            _run(flags=(0, 1, 0), certified=certified, label="certified")
    with pytest.raises(AssertionError, match="left queries to the redo"):
        _run(flags=(0, 0, 3), certified=True)


def test_flag_on_a_query_not_certified_does_not_raise():
    assert _run(flags=(0, 1, 0), certified=[True, False, True])[3].tolist() == [0, 1, 0]
    assert _run(flags=(1, 1, 3), certified=None)[3].tolist() == [1, 1, 3]
    assert _run(flags=(1, 1, 3), certified=[False] * 3)[3].tolist() == [1, 1, 3]
    assert _run(flags=(0, 0, 0), certified=True)[3].tolist() == [0, 0, 0]


# ---- redone -------------------------------------------------------------------------------------------------------------
def _redo(flags, moved, flag=None):
    from vidmem import _lib
    count = [10]

    def check():
        count[0] += moved
        return WANT[0], WANT[1], np.array(flags, dtype=np.int32)
    return redone(check, lambda: count[0], Q, "redo", _lib.VM_FLAG_GAP if flag == "gap" else flag)


def test_redone():
    from vidmem import _lib
    GAP, OVER = _lib.VM_FLAG_GAP, _lib.VM_FLAG_OVERFLOW
    got_r, got_s = _redo([GAP, GAP, GAP], Q, flag="gap")
    assert got_r is WANT[0] and got_s is WANT[1]
    _redo([GAP, OVER, GAP], Q)                                       # no flag demanded: any non-zero one
    with pytest.raises(AssertionError, match="not left to the redo"):
        _redo([GAP, 0, GAP], Q)
    with pytest.raises(AssertionError, match="not left to the redo"):
        _redo([GAP, 0, GAP], Q, flag="gap")
    with pytest.raises(AssertionError, match="for every query"):
        _redo([GAP, OVER, GAP], Q, flag="gap")                       # a flag other than the one demanded
    with pytest.raises(AssertionError, match="neither GAP nor OVERFLOW"):
        _redo([2, GAP, GAP], Q)
    for moved in (0, Q - 1, Q + 1):
        with pytest.raises(AssertionError, match="uncertified counter"):
            _redo([GAP, GAP, GAP], moved, flag="gap")


# ---- to_bits --------------------------------------------------------------------------------------------------------------
def _round_by_hand(x, dtype):
    """The rounding tests/compose_ref.py used to carry: numpy's cast for f16; for bf16 round to nearest even on the fp32
    bit pattern, by adding 0x7FFF plus the lowest kept bit and dropping 16 bits."""
    if dtype == "f16":
        return np.ascontiguousarray(x, dtype=np.float32).astype(np.float16).view(np.uint16)
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7FFF + ((u >> 16) & 1)
    return (u >> 16).astype(np.uint16)


def _widened(dtype):
    """Every finite 16-bit pattern of ``dtype`` as fp32, exactly."""
    p = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    x = p.view(np.float16).astype(np.float32) if dtype == "f16" else (p.astype(np.uint32) << 16).view(np.float32)
    return x[np.isfinite(x)]


def _midpoints(dtype):
    """The fp32 midpoints between neighbouring finite values of ``dtype``, both signs: exact in fp32 (one bit more than
    the 16-bit mantissa, and never below fp32's smallest subnormal)."""
    v = np.unique(_widened(dtype).astype(np.float64))
    mid = (v[:-1] + v[1:]) / 2.0
    assert (mid.astype(np.float32).astype(np.float64) == mid).all()
    return mid.astype(np.float32)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_to_bits_rounds_as_the_rounding_by_hand(dtype):
    with np.errstate(over="ignore"):
        for source in ("f16", "bf16"):
            mid = _midpoints(source)
            inputs = {"patterns": _widened(source), "midpoints": mid,
                      "one ulp below": np.nextafter(mid, np.float32(-np.inf)),
                      "one ulp above": np.nextafter(mid, np.float32(np.inf))}
            for name, x in inputs.items():
                assert x.dtype == np.float32 and x.size > 60000
                want = _round_by_hand(x, dtype)
                finite = (want & (0x7C00 if dtype == "f16" else 0x7F80)) != (0x7C00 if dtype == "f16" else 0x7F80)
                assert finite.sum() > 30000                          # bf16 values beyond f16's range round to inf: left out
                got = to_bits(x, dtype)
                assert got.dtype == np.uint16 and got.shape == x.shape
                differ = np.nonzero((got != want) & finite)[0]
                assert differ.size == 0, (dtype, source, name, x[differ[:5]], got[differ[:5]], want[differ[:5]])
                if source == dtype and name == "patterns":                 # a value of the dtype maps to itself
                    back = got.view(np.float16).astype(np.float32) if dtype == "f16" else (got.astype(np.uint32) << 16).view(np.float32)
                    assert np.array_equal(back, x) and np.array_equal(np.signbit(back), np.signbit(x))
    x64 = np.array([1.0, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -8 + 2.0 ** -9, -65504.0])        # fp64 input: rounded to fp32 first
    assert np.array_equal(to_bits(x64, dtype), _round_by_hand(x64, dtype))
