// Internal definitions shared by the libvidmem translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/vidmem.h"

// Developer A/B switches.  The release library (make / __graft_entry__.build()) compiles every one of them to its
// default: no environment variable selects which kernel produces product results, and no VIDMEM_* name appears in
// libvidmem.so.  tools/dev_build.sh builds with -DVM_DEV_SWITCHES, where each is read from the environment once per
// process.  What a deployment may choose is an explicit per-handle option (vm_encoder_set_option, include/vidmem.h).
//
// The rule: the release library contains exactly the kernels a release call can launch.  A VM_DEV_ENV
// switch may steer between paths the release dispatch reaches as well, or set a number.  A kernel that only a
// non-default value reaches is instantiated by an ordinary `if` on the switch all the same, so it is either compiled,
// with its launch branch, under #ifdef VM_DEV_SWITCHES (events.hip and summary.hip, the simple forms; topk.hip, SCAN_LB),
// or, once the measurement is settled, retired to a patch under tools/experiments/ together with its switch.
#ifdef VM_DEV_SWITCHES
static inline long vm_dev_env_(const char *name, long dflt) {
    const char *e = getenv(name);
    return e ? atol(e) : dflt;
}
#define VM_DEV_ENV(name, dflt) vm_dev_env_("VIDMEM_" name, (dflt))
#else
#define VM_DEV_ENV(name, dflt) ((long)(dflt))
#endif

// One dynamic-LDS grant (vm_lds_opt_in, below): the host address of a kernel instantiation and the bytes this context
// has raised its hipFuncAttributeMaxDynamicSharedMemorySize to.
struct vm_lds_grant {
    const void *kern;
    int bytes;
};
// Slots of the open-addressed table, a power of two.  The library holds well over 200 instantiations that opt in (every
// dtype, epilogue, attention shape, scan plan and search policy); 512 slots, 8 KiB of the context, keep them all, so the
// full-table path below stays an exception.
constexpr int VM_LDS_GRANTS = 512;

struct vm_ctx {
    int device;
    int num_cus;
    char err[512];
    vm_lds_grant lds_grant[VM_LDS_GRANTS];   // all zero = empty, so vm_init's memset builds it
    // optional per-kernel timing (vm_profile_enable): event pool, 2 events + 1 category per launch
    hipEvent_t *prof_ev;
    int *prof_cat;
    int prof_cap, prof_n;
    uint32_t prof_mask;
    double prof_ms[VM_PROF_NCAT];
    int64_t prof_launches[VM_PROF_NCAT];
    // erf-GELU table of the FC1 epilogue (gemm.hip gelu_tab_*; built in vm_init, context.hip): VM_GELU_TAB_N pairs
    // {a, b} with Phi(x) ~ a + b x on the 1/128-wide interval around x = -5 + i/128, device memory
    float *gelu_tab;
};

constexpr int VM_GELU_TAB_N = 1281;                 // x = -5 ... +5 in steps of 1/128
constexpr int VM_GELU_TAB_BYTES = 10256;            // 1281 x 8 B, padded to whole 16-byte pieces

// Brackets the launches inside a scope with two events when profiling is on; free when it is off.
struct vm_prof_scope {
    vm_ctx *ctx;
    hipStream_t st;
    int slot;
    vm_prof_scope(vm_ctx *c, int cat, hipStream_t s) : ctx(c), st(s), slot(-1) {
        if (c && c->prof_ev && c->prof_n < c->prof_cap && ((c->prof_mask >> cat) & 1u)) {
            slot = c->prof_n++;
            c->prof_cat[slot] = cat;
            (void)hipEventRecord(c->prof_ev[2 * slot], s);
        }
    }
    ~vm_prof_scope() {
        if (slot >= 0) (void)hipEventRecord(ctx->prof_ev[2 * slot + 1], st);
    }
};

inline int vm_fail(vm_ctx *ctx, int code, const char *fmt, ...) {
    if (ctx) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
        va_end(ap);
    }
    return code;
}

#define VM_HIP(ctx, call)                                                                              \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return vm_fail((ctx), VM_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),   \
                           __FILE__, __LINE__);                                                        \
    } while (0)

#define VM_LAUNCH_CHECK(ctx)                                                                           \
    do {                                                                                               \
        hipError_t e_ = hipGetLastError();                                                             \
        if (e_ != hipSuccess)                                                                          \
            return vm_fail((ctx), VM_ERR_HIP, "kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), \
                           __FILE__, __LINE__);                                                        \
    } while (0)

// The one dynamic-LDS opt-in: a launch with `bytes` of dynamic LDS calls this first.  The runtime is asked only when
// `bytes` exceeds what this context already granted the kernel, so a kernel costs one call at its first use and one more
// whenever its size grows; a grant is never lowered (it caps launch validation, it is no occupancy input).  The key is
// the host address of the instantiation and the table is the context's: a context belongs to one device and, like its
// err buffer, to one thread at a time.  A full table only means the attribute is set on every call.  The runtime keeps
// one value per kernel and device: a second context on the same device would start from its own empty table and could
// set a smaller one under the first (the Python layer keeps one context per device and process).
inline int vm_lds_opt_in_(vm_ctx *ctx, const void *kern, size_t bytes, const char *who) {
    vm_lds_grant *g = nullptr;
    const size_t h = ((uintptr_t)kern >> 4) * (size_t)0x9E3779B97F4A7C15ull >> 32;
    for (int i = 0; i < VM_LDS_GRANTS && !g; ++i) {
        vm_lds_grant *s = &ctx->lds_grant[(h + i) & (VM_LDS_GRANTS - 1)];
        if (s->kern == kern || !s->kern) g = s;
    }
    if (g && g->kern == kern && (size_t)g->bytes >= bytes) return VM_OK;
    const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess)
        return vm_fail(ctx, VM_ERR_HIP, "%s: LDS opt-in %zu: %s", who, bytes, hipGetErrorString(e));
    if (g) *g = {kern, (int)bytes};
    return VM_OK;
}
template <class K>
int vm_lds_opt_in(vm_ctx *ctx, K kern, size_t bytes, const char *who) {
    return vm_lds_opt_in_(ctx, (const void *)kern, bytes, who);
}

static inline size_t vm_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// score_mode of the top-k entry points: VM_OK, or VM_ERR_INVALID for a value include/vidmem.h does not define
inline int vm_check_score_mode(vm_ctx *ctx, int score_mode) {
    if (score_mode != VM_SCORE_RAW && score_mode != VM_SCORE_UNIT_INTERVAL)
        return vm_fail(ctx, VM_ERR_INVALID, "bad score_mode %d", score_mode);
    return VM_OK;
}

// ---- inline-asm helpers of the LDS-DMA kernels (gemm, attention, topk_emit, topk_gscan) -------------------------
typedef __attribute__((address_space(3))) void *lds_ptr_t;
typedef const __attribute__((address_space(1))) void *gbl_ptr_t;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));  // a native vector: asm operands must be register values

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void lds_write_b32(unsigned addr, unsigned v) {
    asm volatile("ds_write_b32 %0, %1" ::"v"(addr), "v"(v) : "memory");
}

// ---- 16-bit float helpers (device) ------------------------------------------------------------------------
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int DT>
struct vm_elem;  // DT = VM_F16 / VM_BF16
template <>
struct vm_elem<VM_F16> {
    using vec8 = f16x8;
    static __device__ __forceinline__ float to_float(uint16_t b) {
        _Float16 h;
        __builtin_memcpy(&h, &b, 2);
        return (float)h;
    }
    static __device__ __forceinline__ double to_double(uint16_t b) { return (double)to_float(b); }
    static __device__ __forceinline__ uint16_t from_float(float f) {
        _Float16 h = (_Float16)f;  // round-to-nearest-even
        uint16_t b;
        __builtin_memcpy(&b, &h, 2);
        return b;
    }
    // two values -> one packed dword (lo = a): a single v_cvt_pk_f16_f32, same RNE rounding as from_float
    static __device__ __forceinline__ uint32_t pack2(float a, float b) {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        typedef float f2 __attribute__((ext_vector_type(2)));
        const h2 v = __builtin_convertvector(f2{a, b}, h2);
        uint32_t u;
        __builtin_memcpy(&u, &v, 4);
        return u;
    }
    static __device__ __forceinline__ f32x4 mfma16(vec8 a, vec8 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x16 mfma32(vec8 a, vec8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
};
template <>
struct vm_elem<VM_BF16> {
    using vec8 = bf16x8;
    static __device__ __forceinline__ float to_float(uint16_t b) {
        uint32_t u = ((uint32_t)b) << 16;
        return __builtin_bit_cast(float, u);
    }
    static __device__ __forceinline__ double to_double(uint16_t b) { return (double)to_float(b); }
    static __device__ __forceinline__ uint16_t from_float(float f) {
        __bf16 h = (__bf16)f;  // v_cvt_pk_bf16_f32: RNE, NaN stays NaN
        uint16_t b;
        __builtin_memcpy(&b, &h, 2);
        return b;
    }
    static __device__ __forceinline__ uint32_t pack2(float a, float b) {  // v_cvt_pk_bf16_f32
        typedef __bf16 b2 __attribute__((ext_vector_type(2)));
        typedef float f2 __attribute__((ext_vector_type(2)));
        const b2 v = __builtin_convertvector(f2{a, b}, b2);
        uint32_t u;
        __builtin_memcpy(&u, &v, 4);
        return u;
    }
    static __device__ __forceinline__ f32x4 mfma16(vec8 a, vec8 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x16 mfma32(vec8 a, vec8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
};
