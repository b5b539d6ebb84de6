// Context + frame preprocessing.
#include "vm_internal.h"

#include <cmath>
#include <vector>

static thread_local char g_init_err[256] = "";

// The erf-GELU table of the FC1 epilogue (gemm.hip): entry i holds the minimax line {a, b} of Phi(x) = erfc(-x / sqrt 2) / 2
// over [x_i - h/2, x_i + h/2], x_i = -5 + i h, h = 1/128 - the interval whose members round to index i.  The end
// entries are the constants 0 and 1 (|x| >= 5 - h/2: x Phi(x) is within 1.5e-6 of 0 / x there).  In double precision on
// the host, once per context; |x Phi(x) - x (a + b x)| <= 1.0e-6 |x| inside the table (h^2 / 16 x max |Phi''|).
static void build_gelu_table(std::vector<float> &t) {
    t.assign(VM_GELU_TAB_BYTES / 4, 0.f);
    const double h = 1.0 / 128.0;
    auto Phi = [](double x) { return 0.5 * std::erfc(-x * 0.70710678118654752440); };
    for (int i = 0; i < VM_GELU_TAB_N; ++i) {
        double a, b;
        if (i == 0) {
            a = 0.0, b = 0.0;
        } else if (i == VM_GELU_TAB_N - 1) {
            a = 1.0, b = 0.0;
        } else {
            const double xc = -5.0 + i * h, lo = xc - 0.5 * h, hi = xc + 0.5 * h;
            b = (Phi(hi) - Phi(lo)) / (hi - lo);
            double dmin = 1e300, dmax = -1e300;
            for (int j = 0; j <= 64; ++j) {
                const double x = lo + (hi - lo) * j / 64.0, d = Phi(x) - b * x;
                dmin = d < dmin ? d : dmin;
                dmax = d > dmax ? d : dmax;
            }
            a = 0.5 * (dmin + dmax);
        }
        t[2 * i] = (float)a;
        t[2 * i + 1] = (float)b;
    }
}

extern "C" int vm_abi_version(void) { return 4; }

extern "C" int vm_init(int device, vm_ctx **out) {
    if (!out) return VM_ERR_INVALID;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        snprintf(g_init_err, sizeof(g_init_err), "no HIP device visible");
        return VM_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= count) {
        snprintf(g_init_err, sizeof(g_init_err), "device %d out of range (0..%d)", device, count - 1);
        return VM_ERR_INVALID;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return VM_ERR_HIP;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        snprintf(g_init_err, sizeof(g_init_err), "device %d is %s; libvidmem is built for gfx950 only", device,
                 prop.gcnArchName);
        return VM_ERR_NO_DEVICE;
    }
    if (hipSetDevice(device) != hipSuccess) return VM_ERR_HIP;
    vm_ctx *ctx = new vm_ctx();
    memset(ctx, 0, sizeof(*ctx));
    ctx->device = device;
    ctx->prof_mask = 0xffffffffu;
    ctx->num_cus = prop.multiProcessorCount;
    ctx->err[0] = 0;
    {
        std::vector<float> tab;
        build_gelu_table(tab);
        if (hipMalloc((void **)&ctx->gelu_tab, VM_GELU_TAB_BYTES) != hipSuccess ||
            hipMemcpy(ctx->gelu_tab, tab.data(), VM_GELU_TAB_BYTES, hipMemcpyHostToDevice) != hipSuccess) {
            snprintf(g_init_err, sizeof(g_init_err), "device %d: GELU table allocation failed", device);
            if (ctx->gelu_tab) (void)hipFree(ctx->gelu_tab);
            delete ctx;
            return VM_ERR_NOMEM;
        }
    }
    *out = ctx;
    return VM_OK;
}

extern "C" void vm_destroy(vm_ctx *ctx) {
    if (!ctx) return;
    vm_profile_enable(ctx, 0);
    if (ctx->gelu_tab) (void)hipFree(ctx->gelu_tab);
    delete ctx;
}

extern "C" int vm_profile_enable(vm_ctx *ctx, int max_events) {
    if (!ctx) return VM_ERR_INVALID;
    if (ctx->prof_ev) {
        for (int i = 0; i < 2 * ctx->prof_cap; ++i) (void)hipEventDestroy(ctx->prof_ev[i]);
        delete[] ctx->prof_ev;
        delete[] ctx->prof_cat;
        ctx->prof_ev = nullptr;
        ctx->prof_cat = nullptr;
    }
    ctx->prof_cap = ctx->prof_n = 0;
    for (int i = 0; i < VM_PROF_NCAT; ++i) {
        ctx->prof_ms[i] = 0.0;
        ctx->prof_launches[i] = 0;
    }
    if (max_events <= 0) return VM_OK;
    ctx->prof_ev = new hipEvent_t[2 * (size_t)max_events];
    ctx->prof_cat = new int[max_events];
    for (int i = 0; i < 2 * max_events; ++i) VM_HIP(ctx, hipEventCreate(&ctx->prof_ev[i]));
    ctx->prof_cap = max_events;
    return VM_OK;
}

extern "C" int vm_profile_mask(vm_ctx *ctx, uint32_t category_mask) {
    if (!ctx) return VM_ERR_INVALID;
    ctx->prof_mask = category_mask;
    return VM_OK;
}

extern "C" int vm_profile_read(vm_ctx *ctx, double *total_ms, int64_t *launches) {
    if (!ctx || !total_ms || !launches) return VM_ERR_INVALID;
    VM_HIP(ctx, hipDeviceSynchronize());
    for (int i = 0; i < ctx->prof_n; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->prof_ev[2 * i], ctx->prof_ev[2 * i + 1]) == hipSuccess) {
            ctx->prof_ms[ctx->prof_cat[i]] += ms;
            ctx->prof_launches[ctx->prof_cat[i]] += 1;
        }
    }
    ctx->prof_n = 0;
    for (int i = 0; i < VM_PROF_NCAT; ++i) {
        total_ms[i] = ctx->prof_ms[i];
        launches[i] = ctx->prof_launches[i];
        ctx->prof_ms[i] = 0.0;
        ctx->prof_launches[i] = 0;
    }
    return VM_OK;
}

extern "C" const char *vm_last_error(vm_ctx *ctx) { return ctx ? ctx->err : g_init_err; }

// ---------------------------------------------------------------------------------------------------------
// preprocess: uint8 BGR HWC -> normalised 16-bit, bilinear (half-pixel centres, edge clamp), CHW or patch rows.
// Replaces the CPU frame handling of src/pipeline/vlm_extractor.py:110-128.  HBM-bound and tiny next to the
// encoder (150 KB in + 300 KB out per 224x224 frame); one thread = one 16-byte output chunk.
// ---------------------------------------------------------------------------------------------------------
namespace {
struct PreArgs {
    const uint8_t *src;
    void *dst;
    int B, H, W, S, patch, k_pad, layout;
    int src_aligned8;  // ((uintptr_t)src & 7) == 0: the identity fast path may read the frames as uint2
    float ax, ay;      // source/dest scale (W/S, H/S) in fp32
    float a[3], b[3];
};

__device__ __forceinline__ void axis_tap(int d, float scale, int n, int &i0, int &i1, float &lam) {
    float src = __fsub_rn(__fmul_rn(scale, (float)d + 0.5f), 0.5f);
    src = src < 0.f ? 0.f : src;
    int f = (int)floorf(src);
    if (f > n - 1) f = n - 1;
    i0 = f;
    i1 = f + 1 < n ? f + 1 : n - 1;
    lam = src - (float)f;
}

// PATCH / KPAD: compile-time patch edge and padded row length for the two encoder families (16 / 768, 14 / 640), 0 = read
// them from the arguments.  With constants every index division below becomes a multiply-shift; with run-time
// divisors the kernel was integer-division bound (0.58 ms for 880 frames, ~9x its HBM time).
template <int DT, int PATCH, int KPAD>
__global__ void __launch_bounds__(256) preprocess_kernel(PreArgs p0) {
    using E = vm_elem<DT>;
    PreArgs p = p0;
    if (PATCH) {
        p.patch = PATCH;
        p.k_pad = KPAD;
    }
    const int g = p.patch > 0 ? p.S / p.patch : 0;
    const int pp = p.patch * p.patch;
    const int64_t per_frame =
        p.layout == VM_LAYOUT_PATCHES ? (int64_t)g * g * (p.k_pad / 8) : (int64_t)3 * p.S * (p.S / 8);
    const int64_t total = per_frame * p.B;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        int b;
        int64_t r;
        if (total < ((int64_t)1 << 31)) {  // the usual case: 32-bit division (the 64-bit one costs ~100 instructions)
            const unsigned i32 = (unsigned)idx, pf32 = (unsigned)per_frame;
            b = (int)(i32 / pf32);
            r = (int64_t)(i32 - (unsigned)b * pf32);
        } else {
            b = (int)(idx / per_frame);
            r = idx - (int64_t)b * per_frame;
        }
        const uint8_t *frame = p.src + (size_t)b * p.H * p.W * 3;
        uint16_t o8[8];
        if (PATCH == 16 && p.H == p.S && p.W == p.S && p.src_aligned8) {
            // Frames already at the encoder's size (the bench's 224 x 224 input): the bilinear weights are exactly
            // (1, 0), so the result is the source pixel itself - same value, same roundings as the general path below.
            // The 8 outputs of a chunk are 8 consecutive pixels of one channel: 24 contiguous bytes instead of 32
            // single-byte gathers.  Their offset in the buffer, b * S * S * 3 + (oy * S + ox) * 3 with 8 | ox and 8 | S,
            // is a multiple of 8, so they are 8-byte aligned exactly when the caller's pointer is (src_aligned8, set
            // by the host); a frame pointer at any other byte takes the byte loads of the general path.
            constexpr int chunks = KPAD / 8;
            const int patch_idx = (int)(r / chunks);
            const int k0 = (int)(r - (int64_t)patch_idx * chunks) * 8;
            const int c = k0 / (PATCH * PATCH), rem = k0 - c * PATCH * PATCH;
            const int py = rem / PATCH, px = rem - py * PATCH;
            const int oy = (patch_idx / g) * PATCH + py, ox = (patch_idx % g) * PATCH + px;
            const uint2 *src = reinterpret_cast<const uint2 *>(frame + ((size_t)oy * p.W + ox) * 3);
            const uint2 w0 = src[0], w1 = src[1], w2 = src[2];
            const uint32_t words[7] = {w0.x, w0.y, w1.x, w1.y, w2.x, w2.y, 0u};
            const unsigned ch = 2 - c;  // output RGB <- input BGR: shift the window by ch bytes (v_alignbyte_b32),
            uint32_t sh[6];             // then every pixel sits at a compile-time byte position 3e
#pragma unroll
            for (int i = 0; i < 6; ++i) sh[i] = __builtin_amdgcn_alignbyte(words[i + 1], words[i], ch);
            const float ac = p.a[c], bc = p.b[c];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float pix = (float)((sh[(3 * e) >> 2] >> (((3 * e) & 3) * 8)) & 0xffu);
                o8[e] = E::from_float(__fadd_rn(__fmul_rn(pix, ac), bc));
            }
            uint4 out;
            __builtin_memcpy(&out, o8, 16);
            reinterpret_cast<uint4 *>(p.dst)[idx] = out;
            continue;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            int c, oy, ox;
            bool pad = false;
            if (p.layout == VM_LAYOUT_PATCHES) {
                const int chunks = p.k_pad / 8;
                const int patch_idx = (int)(r / chunks);
                const int k = (int)(r - (int64_t)patch_idx * chunks) * 8 + e;
                pad = k >= 3 * pp;
                c = k / pp;
                const int rem = k - c * pp;
                const int py = rem / p.patch, px = rem - py * p.patch;
                oy = (patch_idx / g) * p.patch + py;
                ox = (patch_idx % g) * p.patch + px;
            } else {
                const int row_chunks = p.S / 8;
                c = (int)(r / ((int64_t)p.S * row_chunks));
                const int64_t r2 = r - (int64_t)c * p.S * row_chunks;
                oy = (int)(r2 / row_chunks);
                ox = (int)(r2 - (int64_t)oy * row_chunks) * 8 + e;
            }
            float v = 0.f;
            if (!pad) {
                int y0, y1, x0, x1;
                float ly, lx;
                axis_tap(oy, p.ay, p.H, y0, y1, ly);
                axis_tap(ox, p.ax, p.W, x0, x1, lx);
                const int ch = 2 - c;  // output RGB <- input BGR
                const float p00 = (float)frame[((size_t)y0 * p.W + x0) * 3 + ch];
                const float p01 = (float)frame[((size_t)y0 * p.W + x1) * 3 + ch];
                const float p10 = (float)frame[((size_t)y1 * p.W + x0) * 3 + ch];
                const float p11 = (float)frame[((size_t)y1 * p.W + x1) * 3 + ch];
                // no FMA contraction: same roundings as the oracle's numpy expression
                const float top = __fadd_rn(__fmul_rn(1.f - lx, p00), __fmul_rn(lx, p01));
                const float bot = __fadd_rn(__fmul_rn(1.f - lx, p10), __fmul_rn(lx, p11));
                const float val = __fadd_rn(__fmul_rn(1.f - ly, top), __fmul_rn(ly, bot));
                v = __fadd_rn(__fmul_rn(val, p.a[c]), p.b[c]);
            }
            o8[e] = E::from_float(v);
        }
        uint4 out;
        __builtin_memcpy(&out, o8, 16);
        reinterpret_cast<uint4 *>(p.dst)[idx] = out;
    }
}
}  // namespace

extern "C" int vm_preprocess(vm_ctx *ctx, const uint8_t *frames, int B, int H, int W, const float mean[3],
                             const float std[3], int out_S, int dtype, int layout, int patch, int k_pad,
                             void *out, void *stream) {
    if (!ctx) return VM_ERR_INVALID;
    if (!frames || !out || !mean || !std || B <= 0 || H <= 0 || W <= 0)
        return vm_fail(ctx, VM_ERR_INVALID, "vm_preprocess: bad arguments");
    if (out_S <= 0 || out_S % 8 != 0) return vm_fail(ctx, VM_ERR_UNSUPPORTED, "out_S=%d must be a multiple of 8", out_S);
    if (dtype != VM_F16 && dtype != VM_BF16) return vm_fail(ctx, VM_ERR_INVALID, "bad dtype %d", dtype);
    if ((uintptr_t)out & 15) return vm_fail(ctx, VM_ERR_INVALID, "vm_preprocess: out must be 16-byte aligned");
    PreArgs p;
    p.src = frames;
    p.dst = out;
    p.B = B;
    p.H = H;
    p.W = W;
    p.S = out_S;
    p.layout = layout;
    p.src_aligned8 = ((uintptr_t)frames & 7) == 0;
    p.patch = 0;
    p.k_pad = 0;
    if (layout == VM_LAYOUT_PATCHES) {
        if (patch <= 0 || out_S % patch != 0 || k_pad % 8 != 0 || k_pad < 3 * patch * patch)
            return vm_fail(ctx, VM_ERR_INVALID, "vm_preprocess: patch=%d k_pad=%d do not fit S=%d", patch, k_pad,
                           out_S);
        p.patch = patch;
        p.k_pad = k_pad;
    } else if (layout != VM_LAYOUT_CHW) {
        return vm_fail(ctx, VM_ERR_INVALID, "bad layout %d", layout);
    }
    p.ax = (float)W / (float)out_S;
    p.ay = (float)H / (float)out_S;
    for (int c = 0; c < 3; ++c) {
        if (!(std[c] > 0.f)) return vm_fail(ctx, VM_ERR_INVALID, "std[%d] must be > 0", c);
        p.a[c] = 1.0f / (255.0f * std[c]);
        p.b[c] = -mean[c] / std[c];
    }
    const int64_t per_frame = layout == VM_LAYOUT_PATCHES ? (int64_t)(out_S / patch) * (out_S / patch) * (k_pad / 8)
                                                          : (int64_t)3 * out_S * (out_S / 8);
    const int64_t total = per_frame * B;
    int64_t blocks = (total + 255) / 256;
    const int64_t cap = (int64_t)ctx->num_cus * 16;
    if (blocks > cap) blocks = cap;
    hipStream_t st = (hipStream_t)stream;
    vm_prof_scope prof(ctx, VM_PROF_PREPROCESS, st);
    const bool p16 = layout == VM_LAYOUT_PATCHES && patch == 16 && k_pad == 768;
    const bool p14 = layout == VM_LAYOUT_PATCHES && patch == 14 && k_pad == 640;
#define VM_PRE(DT)                                                                      \
    do {                                                                                \
        if (p16) preprocess_kernel<DT, 16, 768><<<(unsigned)blocks, 256, 0, st>>>(p);   \
        else if (p14) preprocess_kernel<DT, 14, 640><<<(unsigned)blocks, 256, 0, st>>>(p); \
        else preprocess_kernel<DT, 0, 0><<<(unsigned)blocks, 256, 0, st>>>(p);          \
    } while (0)
    if (dtype == VM_F16)
        VM_PRE(VM_F16);
    else
        VM_PRE(VM_BF16);
#undef VM_PRE
    VM_LAUNCH_CHECK(ctx);
    return VM_OK;
}
