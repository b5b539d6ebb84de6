"""GPU: vm_preprocess against its oracle, bit for bit, on every kernel branch (DESIGN.md "Preprocess, bit for bit").

Every row of tests/preprocess_ref.py CASES goes through the C ABI directly (a Context, no encoder, so any S / patch /
k_pad is reachable): the int16 bit patterns of the whole output must equal those of the oracle's fp32 output cast to the
case's type, with no allowance; pad columns are the +0 pattern; the output lies between two 256-byte sentinel regions that
must stay untouched (the frames are followed by one too, which only keeps the allocation's shape fixed); the call is made
twice on the current stream and once on another stream and must give the same bits each time.  Frame pointers 1, 3 and 5
bytes into a buffer are cases of the table.  The grid-stride wrap cases take their batch from the device: the smallest B
whose chunks exceed twice the threads of the capped grid (16 blocks per CU, 256 threads).  FrameEncoder.preprocess is
held to the same bits for the two product specs, which pins the wrapper's mean / std / patch_k wiring, and every rejected
argument set must return its documented status, say why, and leave the output alone.

tests/test_preprocess_cpu.py proves that the table holds the values a wrong cast, clamp or index would change.

Out of scope: the branch for total >= 2^31 chunks (64-bit division) needs an output of 32 GiB.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from tests import preprocess_ref as P
from tests.support import TD

pytestmark = pytest.mark.gpu

GUARD = 256                      # bytes before and after the output (and after the frames)
SENT16 = 0x5AA5                  # the guards' int16 pattern
SENT8 = 0xA5


@pytest.fixture(scope="module")
def ctx():
    from vidmem import _lib
    return _lib.Context.get(0)


def _f3(v):
    return (C.c_float * 3)(*v)


class Call:
    """One vm_preprocess call on device buffers carved out of larger ones."""

    def __init__(self, case, fr: np.ndarray):
        from vidmem import _lib
        self.case, self.B = case, fr.shape[0]
        nbytes = fr.size
        self.src = torch.full((case.offset + nbytes + GUARD,), SENT8, dtype=torch.uint8, device="cuda")
        assert self.src.data_ptr() % 256 == 0
        self.src[case.offset:case.offset + nbytes] = torch.from_numpy(np.ascontiguousarray(fr).reshape(-1)).cuda()
        self.n = P.n_out(case, self.B)
        self.dst = torch.full((GUARD // 2 + self.n + GUARD // 2,), SENT16, dtype=torch.int16, device="cuda")
        assert self.dst.data_ptr() % 256 == 0
        mean, std = P.NORMS[case.norm]
        self.args = dict(frames=self.src.data_ptr() + case.offset, B=self.B, H=case.H, W=case.W, mean=_f3(mean),
                         std=_f3(std), S=case.S, dtype=_lib.DTYPES[case.dtype],
                         layout=_lib.VM_LAYOUT_PATCHES if case.layout == "patches" else _lib.VM_LAYOUT_CHW,
                         patch=case.patch, k_pad=case.k_pad, out=self.dst.data_ptr() + GUARD)

    def launch(self, ctx, stream=None, handle="ctx", **override) -> int:
        a = dict(self.args, **override)
        st = torch.cuda.current_stream() if stream is None else stream
        vp = lambda x: None if x is None else C.c_void_p(x)  # noqa: E731
        return int(ctx.L.vm_preprocess(ctx.handle if handle == "ctx" else handle, vp(a["frames"]), a["B"], a["H"], a["W"],
                                       a["mean"], a["std"], a["S"], a["dtype"], a["layout"], a["patch"], a["k_pad"],
                                       vp(a["out"]), C.c_void_p(st.cuda_stream)))

    def read(self):
        """(output bits, whether both guards are intact); synchronises, then refills the output with the sentinel."""
        torch.cuda.synchronize()
        host = self.dst.cpu().numpy()
        g = GUARD // 2
        intact = bool((host[:g] == SENT16).all() and (host[-g:] == SENT16).all())
        src_tail = self.src[-GUARD:].cpu().numpy()
        assert (src_tail == SENT8).all()
        self.dst.fill_(SENT16)
        torch.cuda.synchronize()
        return host[g:-g].copy(), intact


def _same_bits(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{what}: {bad.size} of {want.size} outputs differ; first at {bad[:6].tolist()}: got "
                           f"{[hex(int(v) & 0xFFFF) for v in got[bad[:6]]]} want "
                           f"{[hex(int(v) & 0xFFFF) for v in want[bad[:6]]]}")


def wrap_batch(case) -> int:
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return (2 * 16 * cus * 256) // P.chunks_per_frame(case) + 1


@pytest.mark.parametrize("name", [c.name for c in P.CASES])
def test_output_bits_equal_the_oracle(ctx, name):
    case = P.BY_NAME[name]
    if case.B is P.WRAP:
        B = wrap_batch(case)
        assert P.chunks_per_frame(case) * B > 2 * 16 * 256 * torch.cuda.get_device_properties(0).multi_processor_count
        fr = P.frames(case, B)
        assert not (fr[-1] == fr[:-1]).all(axis=(1, 2, 3)).any()  # the last frame is like no other
        want = P.bits16(P.oracle(case, fr), case.dtype)
    else:
        fr = P.frames(case)
        want = P.bits16(P.oracle_cached(name), case.dtype)
    call = Call(case, fr)
    assert (call.args["frames"] % 8 == 0) == (case.offset % 8 == 0)
    side = torch.cuda.Stream()
    for what, stream in (("first call", None), ("second call", None), ("other stream", side)):
        ctx.check(call.launch(ctx, stream))
        got, intact = call.read()
        _same_bits(got, want, f"{name}, {what}")
        assert intact, f"{name}, {what}: a guard region next to the output was written"
    pad = P.pad_mask(case, call.B)
    assert not got[pad].any(), f"{name}: pad columns are not the +0 pattern"
    assert pad.sum() == (case.k_pad - 3 * case.patch ** 2) * (case.S // case.patch) ** 2 * call.B if case.patch else not pad.any()


# ---- the Python wrapper, two product specs ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encoders():
    from vidmem import specs, synthetic as syn
    from vidmem.encoder import FrameEncoder
    out = {}
    for tag, spec, dtype in (("vit", specs.VIT_B16_224, "f16"), ("clip", specs.CLIP_L14_336, "bf16")):
        spec = dict(spec, layers=1)
        out[tag] = FrameEncoder(spec, syn.encoder_weights(spec, seed=1), dtype=dtype)
    return out


def wrapper_matches_oracle(enc, case, fr=None, want=None, byte_offset=0):
    """FrameEncoder.preprocess of a case's frames (optionally a view byte_offset bytes into a larger buffer) against
    the oracle's bits; also what tests/test_encoder_gpu.py calls."""
    fr = P.frames(case) if fr is None else fr
    want = P.oracle(case, fr) if want is None else want
    buf = torch.zeros(byte_offset + fr.size, dtype=torch.uint8, device="cuda")
    buf[byte_offset:] = torch.from_numpy(np.ascontiguousarray(fr).reshape(-1)).cuda()
    view = buf[byte_offset:].view(fr.shape)
    assert view.is_contiguous() and view.data_ptr() % 8 == byte_offset % 8
    got = enc.preprocess(view, layout=case.layout)
    assert got.dtype == TD[case.dtype] and got.numel() == want.size
    bits = got.contiguous().view(torch.int16).cpu().numpy().reshape(-1)
    _same_bits(bits, P.bits16(want, case.dtype), f"{case.name} through FrameEncoder.preprocess (+{byte_offset} bytes)")
    assert not bits[P.pad_mask(case, fr.shape[0])].any()


@pytest.mark.parametrize("name,byte_offset", [
    ("vit-224x224-patches", 0), ("vit-224x224-patches", 3), ("vit-224x224-chw", 0), ("vit-360x640-patches", 0),
    ("vit-97x131-chw", 5), ("clip-336x336-patches", 0), ("clip-336x336-chw", 1), ("clip-360x640-patches", 0),
    ("clip-97x131-patches", 3), ("clip-7x5-chw", 0)])
def test_frame_encoder_preprocess_bits(encoders, name, byte_offset):
    case = P.BY_NAME[name]
    enc = encoders[name.split("-")[0]]
    assert (enc.spec["image"], enc.spec["patch"], enc.dtype_name) == (case.S, case.patch or enc.spec["patch"], case.dtype)
    assert case.layout == "chw" or enc.patch_k == case.k_pad
    assert tuple(enc.spec["mean"]) == P.NORMS[case.norm][0] and tuple(enc.spec["std"]) == P.NORMS[case.norm][1]
    wrapper_matches_oracle(enc, case, want=P.oracle_cached(name), byte_offset=byte_offset)


# ---- argument checks ----------------------------------------------------------------------------------------------------
INVALID, UNSUPPORTED = -1, -4
REJECTED = [
    # (what, overrides of a sound 20 x 28 -> 32 patch-8 call, status include/vidmem.h documents, a word of the message)
    ("null frames", dict(frames=None), INVALID, "bad arguments"),
    ("null out", dict(out=None), INVALID, "bad arguments"),
    ("null mean", dict(mean=None), INVALID, "bad arguments"),
    ("null std", dict(std=None), INVALID, "bad arguments"),
    ("B = 0", dict(B=0), INVALID, "bad arguments"),
    ("B < 0", dict(B=-2), INVALID, "bad arguments"),
    ("H = 0", dict(H=0), INVALID, "bad arguments"),
    ("W < 0", dict(W=-1), INVALID, "bad arguments"),
    ("out_S = 0", dict(S=0), UNSUPPORTED, "out_S"),
    ("out_S < 0", dict(S=-32), UNSUPPORTED, "out_S"),
    ("out_S % 8", dict(S=28), UNSUPPORTED, "out_S"),
    ("dtype f32", dict(dtype=2), INVALID, "dtype"),
    ("dtype -1", dict(dtype=-1), INVALID, "dtype"),
    ("layout 2", dict(layout=2), INVALID, "layout"),
    ("layout -1", dict(layout=-1), INVALID, "layout"),
    ("patch = 0", dict(patch=0), INVALID, "patch"),
    ("patch < 0", dict(patch=-8), INVALID, "patch"),
    ("S % patch", dict(patch=12, k_pad=432), INVALID, "patch"),
    ("k_pad % 8", dict(k_pad=196), INVALID, "k_pad"),
    ("k_pad < 3 patch^2", dict(k_pad=184), INVALID, "k_pad"),
    ("std = 0", dict(std=(0.5, 0.0, 0.5)), INVALID, "std"),
    ("std < 0", dict(std=(0.5, 0.5, -0.5)), INVALID, "std"),
    ("std NaN", dict(std=(float("nan"), 0.5, 0.5)), INVALID, "std"),
    ("out + 2 bytes", dict(out_shift=2), INVALID, "aligned"),
    ("out + 8 bytes", dict(out_shift=8), INVALID, "aligned"),
]


@pytest.mark.parametrize("what,override,status,word", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejected_arguments(ctx, what, override, status, word):
    case = P.BY_NAME["generic-p8-k256-bf16"]
    call = Call(case, P.frames(case))
    override = dict(override)
    if "std" in override and override["std"] is not None:
        override["std"] = _f3(override["std"])
    if "out_shift" in override:
        override["out"] = call.args["out"] + override.pop("out_shift")
    assert call.launch(ctx, **override) == status, what
    msg = ctx.L.vm_last_error(ctx.handle)
    assert msg and word in msg.decode(), (what, msg)
    got, intact = call.read()
    assert intact and (got == np.int16(SENT16)).all(), f"{what}: a rejected call wrote to the output"
    # the same buffers are sound: the call goes through once the argument is put right
    ctx.check(call.launch(ctx))
    got, intact = call.read()
    _same_bits(got, P.bits16(P.oracle_cached(case.name), case.dtype), "sound call after " + what)
    assert intact


def test_null_context_is_rejected(ctx):
    case = P.BY_NAME["generic-p8-k256-bf16"]
    call = Call(case, P.frames(case))
    assert call.launch(ctx, handle=None) == INVALID
    got, intact = call.read()
    assert intact and (got == np.int16(SENT16)).all()
