"""Loader of the test-only stage shim (tests/native/stage_shim.cpp -> libvidmem_stages.so beside libvidmem.so).

A test helper, not a conftest.  The shim holds C wrappers over the internal launchers of csrc/vm_kernels.h and is linked
against the release library, so ``stages().vmt_gemm(...)`` runs the object code that ships.  It is opened AFTER
``vidmem._lib.lib()``: its DT_NEEDED ``libvidmem.so`` resolves (rpath $ORIGIN) to the file already mapped, and the
``vm_ctx`` of ``vidmem._lib.Context`` is the context every wrapper takes.  A missing shim raises (the build makes it:
``make -C csrc stages``); nothing here skips.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

WRAPPERS = ("vmt_gemm", "vmt_gemm_set_variant", "vmt_attention", "vmt_resid_layernorm", "vmt_embed", "vmt_pool",
            "vmt_text_embed")

EPI_STORE16, EPI_GELU16, EPI_QGELU16, EPI_RESID32, EPI_PATCH, EPI_DELTA16 = 0, 1, 2, 3, 4, 5   # csrc/vm_kernels.h
EPI_NAMES = {0: "STORE16", 1: "GELU16", 2: "QGELU16", 3: "RESID32", 4: "PATCH", 5: "DELTA16"}

_stages: Optional[C.CDLL] = None


def shim_path() -> str:
    from vidmem import _lib
    return os.path.join(os.path.dirname(_lib.LIB_PATH), "libvidmem_stages.so")


def stages() -> C.CDLL:
    global _stages
    if _stages is not None:
        return _stages
    from vidmem import _lib
    _lib.lib()   # the release library first, by the path the package uses
    path = shim_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run __graft_entry__.build() (make -C csrc stages)")
    S = C.CDLL(path)
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    sig = {
        # ctx, dtype, epi, X, W, bias, out16, out32, pos, M, N, K, ldx, ldo, P, T, prof_cat, head_major, hm_rows,
        # hm_stride, stream
        "vmt_gemm": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp] + [i32] * 11 + [vp]),
        "vmt_gemm_set_variant": (None, [i32]),
        # ctx, dtype, qkv, ctx_out, B, T, heads, q_rows, causal, stream
        "vmt_attention": (i32, [vp, i32, vp, vp, i32, i32, i32, i32, i32, vp]),
        # ctx, dtype, x32, delta16, deltaB16, write_x, gamma, beta, eps, out16, rows, H, rstride, lowreg, stream
        "vmt_resid_layernorm": (i32, [vp, i32, vp, vp, vp, i32, vp, vp, f32, vp, i32, i32, i32, i32, vp]),
        # ctx, dtype, patch16, cls, pos, pre_g, pre_b, eps, pre_ln, x32, B, T, H, stream
        "vmt_embed": (i32, [vp, i32, vp, vp, vp, vp, vp, f32, i32, vp, i32, i32, i32, vp]),
        # ctx, dtype, x, delta16, deltaB16, gamma, beta, eps, proj_w, proj_dim, l2, out, B, T, H, pool_row, stream
        "vmt_pool": (i32, [vp, i32, vp, vp, vp, vp, vp, f32, vp, i32, i32, vp, i32, i32, i32, vp, vp]),
        # ctx, ids, tok, pos, vocab, eot_id, x32, pool_row, flags, B, T, H, stream
        "vmt_text_embed": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, i32, i32, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(S, name)   # AttributeError = the shim and this table drifted apart: fail loudly
        fn.restype = res
        fn.argtypes = args
    _stages = S
    return S


def mapped_copies(basename: str) -> int:
    """How many distinct files of this name the process has mapped (by path AND inode: one library = one entry)."""
    seen = set()
    with open("/proc/self/maps") as f:
        for line in f:
            parts = line.split()
            if len(parts) >= 6 and os.path.basename(parts[5]) == basename:
                seen.add((parts[3], parts[4], parts[5]))   # device, inode, path
    return len(seen)


def ptr(t) -> C.c_void_p:
    """Device pointer of a torch tensor (or view), None -> null."""
    return C.c_void_p(None if t is None else t.data_ptr())


class Stages:
    """The wrappers bound to the process's vm_ctx and torch's current stream; a non-zero return code raises."""

    def __init__(self, device: int = 0):
        from vidmem import _lib
        self._lib = _lib
        self.S = stages()
        self.ctx = _lib.Context.get(device)
        import torch
        self.num_cus = torch.cuda.get_device_properties(device).multi_processor_count

    def _st(self):
        return self._lib.current_stream_ptr()

    def gemm(self, dtype, epi, X, W, bias, *, out16=None, out32=None, pos=None, M, N, K, ldx=None, ldo=None, P=0, T=0,
             prof_cat=2, head_major=0, hm_rows=0, hm_stride=0):
        self.ctx.check(self.S.vmt_gemm(self.ctx.handle, self._lib.DTYPES[dtype], epi, ptr(X), ptr(W), ptr(bias),
                                       ptr(out16), ptr(out32), ptr(pos), M, N, K, K if ldx is None else ldx,
                                       N if ldo is None else ldo, P, T, prof_cat, head_major, hm_rows, hm_stride,
                                       self._st()))

    def set_variant(self, v: int):
        self.S.vmt_gemm_set_variant(int(v))

    def attention(self, dtype, qkv, out, B, T, heads, q_rows=0, causal=0):
        self.ctx.check(self.S.vmt_attention(self.ctx.handle, self._lib.DTYPES[dtype], ptr(qkv), ptr(out), B, T, heads,
                                            q_rows, causal, self._st()))

    def resid_layernorm(self, dtype, x32, dA, dB, write_x, gamma, beta, eps, out16, rows, H, rstride=1, lowreg=0):
        self.ctx.check(self.S.vmt_resid_layernorm(self.ctx.handle, self._lib.DTYPES[dtype], ptr(x32), ptr(dA), ptr(dB),
                                                  write_x, ptr(gamma), ptr(beta), eps, ptr(out16), rows, H, rstride,
                                                  lowreg, self._st()))

    def embed(self, dtype, patch16, cls, pos, pre_g, pre_b, eps, pre_ln, x32, B, T, H):
        self.ctx.check(self.S.vmt_embed(self.ctx.handle, self._lib.DTYPES[dtype], ptr(patch16), ptr(cls), ptr(pos),
                                        ptr(pre_g), ptr(pre_b), eps, pre_ln, ptr(x32), B, T, H, self._st()))

    def pool(self, dtype, x, dA, dB, gamma, beta, eps, proj_w, proj_dim, l2, out, B, T, H, pool_row=None):
        self.ctx.check(self.S.vmt_pool(self.ctx.handle, self._lib.DTYPES[dtype], ptr(x), ptr(dA), ptr(dB), ptr(gamma),
                                       ptr(beta), eps, ptr(proj_w), proj_dim, l2, ptr(out), B, T, H, ptr(pool_row),
                                       self._st()))

    def text_embed(self, ids, tok, pos, vocab, eot_id, x32, pool_row, flags, B, T, H):
        self.ctx.check(self.S.vmt_text_embed(self.ctx.handle, ptr(ids), ptr(tok), ptr(pos), vocab, eot_id, ptr(x32),
                                             ptr(pool_row), ptr(flags), B, T, H, self._st()))
