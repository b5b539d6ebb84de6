// Self-attention of the vision encoder, one workgroup per (frame, head), head dim 64, full-row softmax.
//
// Sequence lengths here are 197 (ViT-B/16) and 577 (CLIP-L/14-336): a whole score row fits in registers, so there
// is no online rescaling.  Per wave, 16 query rows at a time:
//   S^T = K . Q^T     MFMA 16x16x32 with K (from LDS) as the A operand and Q (registers) as B: the lane that owns
//                     query column (lane & 15) holds that query's scores for keys 16*kt + 4*(lane>>4) + j, so the
//                     row max / row sum are register reductions plus two shuffles (xor 16, 32).
//   P  = exp2(..)     fp32, masked keys -> 0, packed to 16-bit in exactly the B-operand order of the next MFMA
//                     (k slot j<4 -> key 32ks+4h+j, j>=4 -> key 32ks+16+4h+j-4): no lane movement, no LDS.
//   O^T = V^T . P^T   V stays ROW-major in LDS ([key][64 d], as it is in HBM); the A fragments (4 keys of one d per
//                     lane) come from ds_read_b64_tr_b16, the CDNA4 transposing LDS read: per 16-lane group a
//                     4-row x 16-column block, lane 4q+p supplies the address of row q / columns 4p..4p+3 and lane i
//                     receives column i.  The lane ends up with 4 consecutive d of one query -> 8-byte context stores.
// LDS: K and V tiles [keys][128 B] with the 16-byte chunk index XORed with (key & 7): conflict-free for the
// ds_read_b128 K fragments and for the transposing V reads (8 consecutive keys per 32-lane half).
#include "vm_internal.h"
#include "vm_kernels.h"

namespace {

typedef short s4v __attribute__((__vector_size__(4 * sizeof(short))));
typedef __attribute__((address_space(3))) s4v *lds_s4v_ptr;
typedef const __attribute__((address_space(3))) char *lds_cptr;   // 32-bit LDS byte address that stays one through asm

// "Does any of the eight scores of a 32-key step exceed the row's reference?" as eight compares OR-ed on the scalar
// side.  Written as fmaxf() chains the compiler first canonicalises every MFMA output (v_max_f32 x, x: eleven vector
// instructions for one value); inline-asm v_max3_f32 on MFMA results is not an option - the hazard recogniser does not
// see an asm statement's reads, and the wait states between a matrix write and a vector read are software's job.
__device__ __forceinline__ bool any_above(const f32x4 a, const f32x4 b, float ref) {
    return (a[0] > ref) | (a[1] > ref) | (a[2] > ref) | (a[3] > ref) | (b[0] > ref) | (b[1] > ref) | (b[2] > ref) |
           (b[3] > ref);
}

// Context value of one query and feature: the normalised P.V sum, rounded to fp32 and THEN to the 16-bit output - two
// roundings, spelled out.  Left to the compiler, `from_float(o * inv)` is sometimes one v_fma_mixlo_f16 (a single rounding)
// and sometimes v_pk_mul_f32 + v_cvt_pk_f16_f32, depending on what surrounds it: both fine, but the choice flipped with
// an unrelated edit of the store (round 4) and moved every embedding of the fp16 goldens in the last bit - frame by
// frame by up to 9 % of its distance to the fp32 oracle, the batch from 9.80e-4 to 9.59e-4 (tools/golden_probe.py).  The
// product is therefore pinned as an fp32 value (what oracle/vit_ref's quant-aware mode rounds, too).
template <class E>
__device__ __forceinline__ uint16_t ctx_value(float o, float inv) {
    float prod = o * inv;
    asm("" : "+v"(prod));
    return E::from_float(prod);
}

// One 16-query tile against all keys of the (frame, head) staged in LDS: scores, softmax, P.V, context store.
// CAUSAL (text tower): keys after the lane's query row qrow are masked like keys past T, in every tile, so a row's
// result does not depend on T or on anything behind it as long as the build (NT) is the same.
template <int DT, int NT, bool EXACT, bool CAUSAL = false>
__device__ __forceinline__ void attend_tile(const char *kl, const char *vl, typename vm_elem<DT>::vec8 qa,
                                            typename vm_elem<DT>::vec8 qb, int T, int lane, bool qvalid,
                                            uint16_t *dst_row, int ctx_nt = 0, int qrow = 0) {
    using E = vm_elem<DT>;
    using vec8 = typename E::vec8;
    constexpr int NS = (NT + 1) / 2;  // 32-key steps of the PV product
    const int r16 = lane & 15, h = lane >> 4;
    const float scale_log2e = 0.125f * 1.44269504088896340736f;  // 1/sqrt(64) * log2(e)
    // transposing-read lane constants: lane i of a 16-lane group addresses row q = i>>2, columns 4p.. (p = i&3)
    const int tq = r16 >> 2, tp = r16 & 3;
    // raw scores; key tiles that reach past T get their tail masked (block-uniform test)
    f32x4 s[NT];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        const int key = kt * 16 + r16;
        const vec8 k0 = *reinterpret_cast<const vec8 *>(kl + key * 128 + ((h ^ (key & 7)) << 4));
        const vec8 k1 = *reinterpret_cast<const vec8 *>(kl + key * 128 + (((h + 4) ^ (key & 7)) << 4));
        f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
        a = E::mfma16(k0, qa, a);
        a = E::mfma16(k1, qb, a);
        if (CAUSAL) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int key = kt * 16 + 4 * h + j;
                a[j] = (key < T && key <= qrow) ? a[j] : -INFINITY;   // key 0 always passes: the row max is finite
            }
        } else if (EXACT ? (kt == NT - 1) : (kt * 16 + 16 > T)) {
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = (kt * 16 + 4 * h + j < T) ? a[j] : -INFINITY;
        }
        mx = fmaxf(fmaxf(mx, fmaxf(a[0], a[1])), fmaxf(a[2], a[3]));
        s[kt] = a;
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // exp((s - max) / 8) = exp2(s * c - max * c): one fma + one v_exp per score
    const float neg_mxc = -mx * scale_log2e;
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 c2 = {scale_log2e, scale_log2e}, n2 = {neg_mxc, neg_mxc};
    f32x2 sum2 = {0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        // the fma and the running sum on 2-vectors (v_pk_fma_f32 / v_pk_add_f32); v_exp_f32 is scalar
        f32x2 a01 = __builtin_elementwise_fma(f32x2{s[kt][0], s[kt][1]}, c2, n2);
        f32x2 a23 = __builtin_elementwise_fma(f32x2{s[kt][2], s[kt][3]}, c2, n2);
        a01 = f32x2{__builtin_amdgcn_exp2f(a01.x), __builtin_amdgcn_exp2f(a01.y)};
        a23 = f32x2{__builtin_amdgcn_exp2f(a23.x), __builtin_amdgcn_exp2f(a23.y)};
        sum2 += a01;
        sum2 += a23;
        s[kt] = f32x4{a01.x, a01.y, a23.x, a23.y};
    }
    float sum = sum2.x + sum2.y;
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;

    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NS; ++ks) {
        uint16_t pe[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pe[j] = E::from_float(s[2 * ks][j]);
            pe[4 + j] = (2 * ks + 1 < NT) ? E::from_float(s[2 * ks + 1][j]) : (uint16_t)0;
        }
        vec8 pf;
        __builtin_memcpy(&pf, pe, 16);
        const int key_lo = ks * 32 + 4 * h + tq, key_hi = key_lo + 16;  // (key & 7) is the same for both
        const char *row_lo = vl + key_lo * 128 + (tp & 1) * 8;
        const int sw = key_lo & 7;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const int coff = ((2 * dt + (tp >> 1)) ^ sw) << 4;
            const s4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v_ptr)(row_lo + coff));
            const s4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (lds_s4v_ptr)(row_lo + (2 * ks + 1 < NT ? 16 * 128 : 0) + coff));
            typedef short s8v __attribute__((__vector_size__(8 * sizeof(short))));
            const s8v av = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);  // register pair concatenation
            o[dt] = E::mfma16(__builtin_bit_cast(vec8, av), pf, o[dt]);
        }
        (void)key_hi;
    }
    if (qvalid) {
        uint16_t *dst = dst_row + 4 * h;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            uint16_t oe[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) oe[j] = ctx_value<E>(o[dt][j], inv);
            uint2 pk;
            __builtin_memcpy(&pk, oe, 8);
            typedef unsigned ctx_u32x2 __attribute__((ext_vector_type(2)));
            if (ctx_nt) __builtin_nontemporal_store(ctx_u32x2{pk.x, pk.y}, reinterpret_cast<ctx_u32x2 *>(dst + dt * 16));
            else *reinterpret_cast<uint2 *>(dst + dt * 16) = pk;
        }
    }
}

// Long rows (577 tokens: 37 key tiles): the whole score row does not fit in registers next to the accumulators (148 VGPRs
// of scores alone), so the keys are walked once, 32 at a time, with an ONLINE softmax: exp2((s - m_ref) c) / sum of the
// same is shift-invariant, so any reference m_ref gives the same result up to fp32 / 16-bit roundings.
// LAZY reference: m_ref is not the running maximum but a value the scores may exceed by up to ONLINE_SLACK (in units of
// the exponent, i.e. probabilities up to 2^ONLINE_SLACK before the final division: harmless in fp32 sums and in a 16-bit
// P, whose relative precision does not depend on its magnitude).  The common step therefore needs no cross-lane traffic
// at all: every lane tests its OWN scores against the shared reference (one ballot); only when some score breaks out -
// the first step, and the few later ones where the row maximum grows by more than the slack - are the two shuffles, the
// rescale of the sums and the new reference paid.  (With the reference tied to the exact running maximum every step
// carried a dependent chain max -> shuffle -> max -> shuffle -> ballot of ~300 cycles.)
// Every LDS read of a step is issued up front - the K fragments of both key tiles and the eight transposed V fragments
// (they do not depend on P) - so one LDS latency is exposed per 32 keys instead of six.
// TWO query tiles per wave and walk (32 queries): the K and V fragments of a 32-key step are read from LDS once and feed
// both tiles' MFMAs, and the two tiles' softmax chains (MFMA -> max test -> exp2 -> pack -> MFMA) are independent
// instruction streams inside one wave, so one chain's latencies are covered by the other's work.  Measured (CLIP-L/14-336
// bf16, 448 frames, ms of attention): one tile per walk, 16 waves 26.0; pairs, 8 / 10 / 12 waves 27.4 (before the address
// trimming) / 28.3 / 24.9 - a 4 % gain, i.e. the walk is not latency-bound; what it IS bound by has not been found
// (matrix pipe 24 % busy, LDS ~27 %, the vector port ~65 % by instruction count; the K/V fill of a workgroup is 17 % of
// its life and overlaps nothing).  The one-tile walk, the two-pass softmax before it, the 8- and 10-wave builds and the
// compile-time ablations of this walk are patches now: tools/experiments/attention_retired_variants.patch, DESIGN.md 4.3.
template <int DT, int NT, bool EXACT>
__device__ __forceinline__ void attend_pair_online(const char *kl, const char *vl,
                                                   const typename vm_elem<DT>::vec8 (&qa)[2],
                                                   const typename vm_elem<DT>::vec8 (&qb)[2], int T, int lane,
                                                   const bool (&qvalid)[2], uint16_t *const (&dst_row)[2]) {
    using E = vm_elem<DT>;
    using vec8 = typename E::vec8;
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    constexpr int NS = (NT + 1) / 2;
    constexpr float ONLINE_SLACK = 6.0f;
    const int r16 = lane & 15, h = lane >> 4;
    const int tq = r16 >> 2, tp = r16 & 3;
    const float scale_log2e = 0.125f * 1.44269504088896340736f;
    const f32x2 c2 = {scale_log2e, scale_log2e};
    const char *p0 = kl + r16 * 128 + ((h ^ (r16 & 7)) << 4);
    const char *p1 = kl + r16 * 128 + (((h + 4) ^ (r16 & 7)) << 4);
    const int vsw = (4 * h + tq) & 7;
    const char *vrow = vl + (4 * h + tq) * 128 + (tp & 1) * 8;
    int voff[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) voff[dt] = ((2 * dt + (tp >> 1)) ^ vsw) << 4;
    float run_m[2] = {-1e30f, -1e30f}, run_hi[2] = {-1e30f, -1e30f};
    f32x2 n2[2] = {{1e30f * scale_log2e, 1e30f * scale_log2e}, {1e30f * scale_log2e, 1e30f * scale_log2e}};
    f32x2 sum2[2] = {{0.f, 0.f}, {0.f, 0.f}};
    f32x4 o[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[t][dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    lds_cptr kp0 = (lds_cptr)p0, kp1 = (lds_cptr)p1;   // running LDS pointers: one 32-key step = 4 KiB
    lds_cptr vp[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) vp[dt] = (lds_cptr)(vrow + voff[dt]);
    auto step = [&](int ks, bool masked0, bool has1, bool masked1) {
        const int hi_off = has1 ? 16 * 128 : 0;
        typedef const __attribute__((address_space(3))) vec8 *lds_vec8_ptr;
        const vec8 ka0 = *(lds_vec8_ptr)(kp0);
        const vec8 ka1 = *(lds_vec8_ptr)(kp1);
        const vec8 kb0 = *(lds_vec8_ptr)(kp0 + (has1 ? 2048 : 0));
        const vec8 kb1 = *(lds_vec8_ptr)(kp1 + (has1 ? 2048 : 0));
        s4v vlo[4], vhi[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            vlo[dt] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v_ptr)(vp[dt]));
            vhi[dt] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v_ptr)(vp[dt] + hi_off));
        }
        kp0 += 4096;
        kp1 += 4096;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) vp[dt] += 4096;
        // keep them as six loop-carried registers (the compiler otherwise re-derives every address from one induction
        // variable plus the image offset, which does not fit a ds_read immediate: 14 adds per step instead of 6)
        asm volatile("" : "+v"(kp0), "+v"(kp1), "+v"(vp[0]), "+v"(vp[1]), "+v"(vp[2]), "+v"(vp[3]));
        f32x4 a[2][2];
        bool out_of_slack = false;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            a[t][0] = E::mfma16(ka0, qa[t], f32x4{0.f, 0.f, 0.f, 0.f});
            a[t][0] = E::mfma16(ka1, qb[t], a[t][0]);
            a[t][1] = E::mfma16(kb0, qa[t], f32x4{0.f, 0.f, 0.f, 0.f});
            a[t][1] = E::mfma16(kb1, qb[t], a[t][1]);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (masked0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) a[t][0][j] = ((2 * ks) * 16 + 4 * h + j < T) ? a[t][0][j] : -INFINITY;
            }
            if (!has1) {
                a[t][1] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            } else if (masked1) {
#pragma unroll
                for (int j = 0; j < 4; ++j) a[t][1][j] = ((2 * ks + 1) * 16 + 4 * h + j < T) ? a[t][1][j] : -INFINITY;
            }
            out_of_slack |= any_above(a[t][0], a[t][1], run_hi[t]);
        }
        if (__ballot(out_of_slack) != 0ull) {  // wave-uniform, rare after the first step
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const float lm_own = fmaxf(fmaxf(fmaxf(a[t][0][0], a[t][0][1]), fmaxf(a[t][0][2], a[t][0][3])),
                                           fmaxf(fmaxf(a[t][1][0], a[t][1][1]), fmaxf(a[t][1][2], a[t][1][3])));
                float lm = fmaxf(lm_own, __shfl_xor(lm_own, 16, 64));
                lm = fmaxf(lm, __shfl_xor(lm, 32, 64));
                // a row whose scores stayed within its slack keeps its reference: f = 1 exactly
                const float m_new = lm > run_hi[t] ? lm : run_m[t];
                const float f = __builtin_amdgcn_exp2f((run_m[t] - m_new) * scale_log2e);
                sum2[t] *= f32x2{f, f};
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) o[t][dt] *= f32x4{f, f, f, f};
                run_m[t] = m_new;
                run_hi[t] = m_new + ONLINE_SLACK / scale_log2e;
                const float neg = -m_new * scale_log2e;
                n2[t] = f32x2{neg, neg};
            }
        }
        // Tile 0's probabilities first, then its four P.V MFMAs with tile 1's exponentials BETWEEN them (two 8-cycle
        // transcendentals per 16-cycle MFMA), then tile 1's MFMAs.  With the MFMAs of both tiles paired per V fragment
        // (the natural loop nest) every exponential of the step had to be finished before the second MFMA could issue:
        // 16 v_exp + 8 converts with the matrix pipe idle, then 8 MFMAs with the vector pipe idle.
        auto softmax_pack = [&](int t) -> vec8 {
            uint16_t pe[8];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                f32x2 p01 = __builtin_elementwise_fma(f32x2{a[t][u][0], a[t][u][1]}, c2, n2[t]);
                f32x2 p23 = __builtin_elementwise_fma(f32x2{a[t][u][2], a[t][u][3]}, c2, n2[t]);
                p01 = f32x2{__builtin_amdgcn_exp2f(p01.x), __builtin_amdgcn_exp2f(p01.y)};
                p23 = f32x2{__builtin_amdgcn_exp2f(p23.x), __builtin_amdgcn_exp2f(p23.y)};
                sum2[t] += p01 + p23;
                pe[4 * u + 0] = E::from_float(p01.x);
                pe[4 * u + 1] = E::from_float(p01.y);
                pe[4 * u + 2] = E::from_float(p23.x);
                pe[4 * u + 3] = E::from_float(p23.y);
            }
            vec8 pf;
            __builtin_memcpy(&pf, pe, 16);
            return pf;
        };
        vec8 av[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
            av[dt] = __builtin_bit_cast(vec8, __builtin_shufflevector(vlo[dt], vhi[dt], 0, 1, 2, 3, 4, 5, 6, 7));
        const vec8 pf0 = softmax_pack(0);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[0][dt] = E::mfma16(av[dt], pf0, o[0][dt]);
        const vec8 pf1 = softmax_pack(1);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[1][dt] = E::mfma16(av[dt], pf1, o[1][dt]);
        // schedule of the region above: (1 MFMA, 2 transcendentals) x 4 - tile 0's MFMAs over tile 1's exponentials
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x400, 2, 0);
        }
    };
    constexpr int FULL_STEPS = EXACT ? (NT - 1) / 2 : 0;
    int ks = 0;
#pragma unroll 1
    for (; ks < FULL_STEPS; ++ks) step(ks, false, true, false);
#pragma unroll 1
    for (; ks < NS; ++ks) step(ks, true, 2 * ks + 1 < NT, true);

#pragma unroll
    for (int t = 0; t < 2; ++t) {
        float sum = sum2[t].x + sum2[t].y;
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.0f / sum;
        if (qvalid[t]) {
            uint16_t *dst = dst_row[t] + 4 * h;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                uint16_t oe[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) oe[j] = ctx_value<E>(o[t][dt][j], inv);
                uint2 pk;
                __builtin_memcpy(&pk, oe, 8);
                *reinterpret_cast<uint2 *>(dst + dt * 16) = pk;
            }
        }
    }
}

// One workgroup of NW waves per (frame, head), every wave walks PAIRS of query tiles (attend_pair_online): pairs wave,
// wave + NW, ...  With 37 tiles = 19 pairs and 12 waves seven waves take two pairs and five take one (16 waves with
// one tile per walk: five waves take three tiles while eleven take two).
template <int DT, int NT, bool EXACT, int NW>
__global__ void __launch_bounds__(NW * 64, 1)
    attention_pair_kernel(const uint16_t *__restrict__ qkv, uint16_t *__restrict__ ctx_out, int T, int heads,
                          int qt_lim) {
    using E = vm_elem<DT>;
    using vec8 = typename E::vec8;
    constexpr int ROWS = NT * 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *kl = smem, *vl = smem + (size_t)ROWS * 128;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, h = lane >> 4;
    const int b = blockIdx.x / heads, head = blockIdx.x - b * heads;
    const int H = heads * 64;
    const size_t M = (size_t)(gridDim.x / heads) * T;
    auto block = [&](int part) { return qkv + ((size_t)(part * heads + head) * M + (size_t)b * T) * 64; };
    auto load_q = [&](int qt, vec8 &q0, vec8 &q1) {
        int qtok = qt * 16 + r16;
        if (qtok > T - 1) qtok = T - 1;
        const uint16_t *qp = block(0) + (size_t)qtok * 64;
        q0 = __builtin_bit_cast(vec8, *reinterpret_cast<const uint4 *>(qp + 8 * h));
        q1 = __builtin_bit_cast(vec8, *reinterpret_cast<const uint4 *>(qp + 32 + 8 * h));
    };
    const int srow = lane >> 3, scp = lane & 7;
    auto stage = [&](int part, char *dst) {  // rows past T re-read row T-1 (masked / P = 0 later)
        const char *src = reinterpret_cast<const char *>(block(part));
#pragma unroll 4
        for (int grp = wave; grp < ROWS / 8; grp += NW) {
            int key = grp * 8 + srow;
            key = key > T - 1 ? T - 1 : key;
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(src + (size_t)key * 128 + ((scp ^ srow) << 4)),
                                             (lds_ptr_t)(dst + grp * 1024), 16, 0, 2);  // nt: read once
        }
    };
    // The fill is 25 % of this kernel with nothing to overlap it (compile-time ablation table).  Round 4
    // tried to hide it: the K / V rows in four chunks issued by five loader waves (the ones that walk one pair where
    // the others walk two), the other waves starting after chunk 0 and meeting the loaders at one barrier per chunk.
    // Bit-identical, and 7-9 % SLOWER (CLIP-L/14-336, 224 frames: 24.0 -> 26.3 ms of attention per two passes): the
    // chunk barriers keep the seven walking waves in lockstep and the loaders' own walk starts no earlier than before.
    // The whole-fill barrier stays (tools/experiments/attention_pair_chunked_fill.patch).
    const int npairs = (qt_lim + 1) / 2;
    vec8 qa[2], qb[2];
    if (wave < npairs) {
        load_q(2 * wave, qa[0], qb[0]);
        load_q(2 * wave + 1, qa[1], qb[1]);
    }
    stage(1, kl);
    stage(2, vl);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int pr = wave; pr < npairs; pr += NW) {
        bool qvalid[2];
        uint16_t *dst[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int qt = 2 * pr + t;
            const int qtok = qt * 16 + r16;
            qvalid[t] = qt < qt_lim && qtok < T;
            dst[t] = ctx_out + ((size_t)b * T + (qvalid[t] ? qtok : 0)) * H + head * 64;
        }
        const vec8 ca[2] = {qa[0], qa[1]}, cb[2] = {qb[0], qb[1]};
        if (pr + NW < npairs) {
            load_q(2 * (pr + NW), qa[0], qb[0]);
            load_q(2 * (pr + NW) + 1, qa[1], qb[1]);
        }
        attend_pair_online<DT, NT, EXACT>(kl, vl, ca, cb, T, lane, qvalid, dst);
    }
}

// PERSISTENT form of the pair kernel (round 4): one workgroup per CU walks (frame, head) items, and the NEXT item's K / V
// rows travel HBM -> registers while the current item is still being walked.  With 19 pairs on 12 waves seven waves walk
// two pairs and five walk one (in the last layer, CLS rows only: one wave walks, eleven have nothing): the waves that
// are done early hold no live state, so each of them fetches its share of the next item's 148 KB into registers
// (30 x 16 B per lane for five waves) - plain global loads, no LDS needed while the others still read the current
// images - and after the barrier that ends the walk writes them to LDS with ds_write_b128 (~0.5 us).  The K / V fill,
// 25 % of the one-workgroup-per-item kernel with nothing to overlap it (ablation table; a chunked fill
// by loader waves was 7-9 % slower), leaves the critical path.  Same LDS image (row r at r * 128, 16-byte chunk c
// holding source chunk c ^ (r & 7), rows past T re-reading row T - 1), same walk: bit-identical outputs.
// PF_MAX: 16-byte registers a prefetching wave may hold; the launcher picks this kernel only when the idle waves' share
// fits (pair counts 1-7 and 13-19 with 12 waves).
template <int DT, int NT, bool EXACT, int NW, int PF_MAX>
__global__ void __launch_bounds__(NW * 64, 1)
    attention_pair_persist_kernel(const uint16_t *__restrict__ qkv, uint16_t *__restrict__ ctx_out, int T, int heads,
                                  int qt_lim, int items) {
    using E = vm_elem<DT>;
    using vec8 = typename E::vec8;
    constexpr int ROWS = NT * 16;
    constexpr int CHUNKS = 2 * ROWS * 8;   // 16-byte chunks of the K image followed by the V image
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *kl = smem, *vl = smem + (size_t)ROWS * 128;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, h = lane >> 4;
    const int H = heads * 64;
    const size_t M = (size_t)(items / heads) * T;
    if ((int)blockIdx.x >= items) return;
    auto block = [&](int item, int part) {
        const int b = item / heads, head = item - b * heads;
        return qkv + ((size_t)(part * heads + head) * M + (size_t)b * T) * 64;
    };
    auto load_q = [&](int item, int qt, vec8 &q0, vec8 &q1) {
        int qtok = qt * 16 + r16;
        if (qtok > T - 1) qtok = T - 1;
        const uint16_t *qp = block(item, 0) + (size_t)qtok * 64;
        q0 = __builtin_bit_cast(vec8, *reinterpret_cast<const uint4 *>(qp + 8 * h));
        q1 = __builtin_bit_cast(vec8, *reinterpret_cast<const uint4 *>(qp + 32 + 8 * h));
    };
    const int npairs = (qt_lim + 1) / 2;
    const int maxc = (npairs + NW - 1) / NW;                 // pairs of the busiest wave
    int w0 = npairs - (maxc - 1) * NW;                       // first wave with fewer pairs than that
    if (w0 >= NW) w0 = 0;                                    // none: every wave fetches after its walk (no overlap)
    const int P = NW - w0, pw = wave - w0;                   // prefetching waves, this wave's rank among them
    // (PF_MAX * P >= CHUNKS / 64: checked by the launcher)

    int item = blockIdx.x;
    vec8 qa[2], qb[2];
    if (wave < npairs) {
        load_q(item, 2 * wave, qa[0], qb[0]);
        load_q(item, 2 * wave + 1, qa[1], qb[1]);
    }
    {   // first item: LDS-DMA fill by every wave, as in the one-item kernel
        const int srow = lane >> 3, scp = lane & 7;
#pragma unroll
        for (int part = 1; part <= 2; ++part) {
            const char *src = reinterpret_cast<const char *>(block(item, part));
            char *dst = part == 1 ? kl : vl;
#pragma unroll 4
            for (int grp = wave; grp < ROWS / 8; grp += NW) {
                int key = grp * 8 + srow;
                key = key > T - 1 ? T - 1 : key;
                __builtin_amdgcn_global_load_lds((gbl_ptr_t)(src + (size_t)key * 128 + ((scp ^ srow) << 4)),
                                                 (lds_ptr_t)(dst + grp * 1024), 16, 0, 2);  // nt: read once
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    while (true) {
        const int next = item + (int)gridDim.x;
        const bool has_next = next < items;
        const int b = item / heads, head = item - b * heads;
        for (int pr = wave; pr < npairs; pr += NW) {
            bool qvalid[2];
            uint16_t *dst[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int qt = 2 * pr + t;
                const int qtok = qt * 16 + r16;
                qvalid[t] = qt < qt_lim && qtok < T;
                dst[t] = ctx_out + ((size_t)b * T + (qvalid[t] ? qtok : 0)) * H + head * 64;
            }
            const vec8 ca[2] = {qa[0], qa[1]}, cb[2] = {qb[0], qb[1]};
            if (pr + NW < npairs) {            // this wave's next pair of the same item ...
                load_q(item, 2 * (pr + NW), qa[0], qb[0]);
                load_q(item, 2 * (pr + NW) + 1, qa[1], qb[1]);
            } else if (has_next && pw < 0) {   // ... or its first pair of the next item: in flight during this walk
                load_q(next, 2 * wave, qa[0], qb[0]);   // (a prefetching wave loads it behind its LDS writes instead:
                load_q(next, 2 * wave + 1, qa[1], qb[1]);   // 16 registers it needs for the rows, latency it can afford)
            }
            attend_pair_online<DT, NT, EXACT>(kl, vl, ca, cb, T, lane, qvalid, dst);
        }
        if (!has_next) break;
        // the waves that are done early fetch the next item's rows into registers while the others still walk.  A wave
        // instruction moves one 8-row group g of the combined K | V image (1 KiB): which image, and the group's first
        // row, are wave-uniform; per lane only the row inside the group and its swizzled chunk (both fixed).
        // Two barriers either way: (1) every wave's reads of the current images have returned (their MFMAs consumed
        // them) - raw s_barrier, no vmcnt wait for the walkers' context stores; (2) the new images are in LDS.
        if (pw >= 0) {
            typedef unsigned pf_u32x4 __attribute__((ext_vector_type(4)));
            pf_u32x4 buf[PF_MAX];
            const char *kbase = reinterpret_cast<const char *>(block(next, 1));
            const char *vbase = reinterpret_cast<const char *>(block(next, 2));
            int lrow = lane >> 3;
            asm volatile("" : "+v"(lrow));   // opaque per item: keeps hoisted offsets from living across the walk
            const unsigned lane_term = (unsigned)(((lane & 7) ^ lrow) << 4);
#pragma unroll
            for (int j = 0; j < PF_MAX; ++j) {   // straight-line: under per-j branches the compiler keeps buf in scratch
                int g = __builtin_amdgcn_readfirstlane(j * P + pw);
                g = g < CHUNKS / 64 ? g : CHUNKS / 64 - 1;   // past the end: the last group again (same bytes, same place)
                const bool is_v = g >= ROWS / 8;
                int key = (is_v ? g - ROWS / 8 : g) * 8 + lrow;
                key = key > T - 1 ? T - 1 : key;
                const char *src = (is_v ? vbase : kbase) + ((unsigned)key * 128u + lane_term);
                buf[j] = __builtin_nontemporal_load(reinterpret_cast<const pf_u32x4 *>(src));
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
            for (int j = 0; j < PF_MAX; ++j) {
                int g = __builtin_amdgcn_readfirstlane(j * P + pw);
                g = g < CHUNKS / 64 ? g : CHUNKS / 64 - 1;
                *reinterpret_cast<pf_u32x4 *>(smem + (size_t)g * 1024 + lane * 16) = buf[j];
            }
            if (wave < npairs) {
                load_q(next, 2 * wave, qa[0], qb[0]);
                load_q(next, 2 * wave + 1, qa[1], qb[1]);
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        } else {
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        }
        item = next;
    }
}

// The launches of launch_long, one per kernel: lds = the K | V image, ql = query tiles wanted (<= NT).  Twelve waves, three
// per SIMD (NW stays a template parameter of the kernels, whose fill and pair loops are written for any count).
template <int DT, int NT, bool EXACT>
int launch_pair(vm_ctx *ctx, const uint16_t *qkv, uint16_t *out, int items, int T, int heads, hipStream_t st, int ql,
                size_t lds) {
    auto kern = attention_pair_kernel<DT, NT, EXACT, 12>;
    if (int r = vm_lds_opt_in(ctx, kern, lds, "vm_attention")) return r;
    kern<<<items, 12 * 64, lds, st>>>(qkv, out, T, heads, ql);
    VM_LAUNCH_CHECK(ctx);
    return VM_OK;
}
template <int DT, int NT, bool EXACT, int PF>
int launch_persist(vm_ctx *ctx, const uint16_t *qkv, uint16_t *out, int items, int T, int heads, hipStream_t st, int ql,
                   size_t lds) {
    auto kern = attention_pair_persist_kernel<DT, NT, EXACT, 12, PF>;
    if (int r = vm_lds_opt_in(ctx, kern, lds, "vm_attention")) return r;
    kern<<<items < ctx->num_cus ? items : ctx->num_cus, 12 * 64, lds, st>>>(qkv, out, T, heads, ql, items);
    VM_LAUNCH_CHECK(ctx);
    return VM_OK;
}

template <int DT, int NT, bool EXACT>
int launch_long(vm_ctx *ctx, const uint16_t *qkv, uint16_t *out, int B, int T, int heads, hipStream_t st, int qt_lim) {
    const size_t lds = (size_t)NT * 16 * 128 * 2;
    vm_prof_scope prof(ctx, VM_PROF_ATTENTION, st);
    const int ql = qt_lim < NT ? qt_lim : NT, items = B * heads;
    // persistent walk with the next item's rows prefetched into the idle waves' registers: when their share fits
    static const int persist_env = (int)VM_DEV_ENV("ATTN_PERSIST", 1);
    const int npairs = (ql + 1) / 2, maxc = (npairs + 11) / 12;
    int w0 = npairs - (maxc - 1) * 12;
    if (w0 >= 12) w0 = 0;
    constexpr int GROUPS = 2 * NT * 16 / 8;             // 8-row groups of the K | V image
    constexpr int PF_FEW = (GROUPS + 4) / 5;            // 16-byte registers per lane with five prefetching waves
    constexpr int PF_MANY = (GROUPS + 10) / 11;         // ... with eleven (one pair to walk: the last layer's CLS rows)
    const int pf = (GROUPS + (12 - w0) - 1) / (12 - w0);
    if (persist_env && pf <= PF_MANY) return launch_persist<DT, NT, EXACT, PF_MANY>(ctx, qkv, out, items, T, heads, st, ql, lds);
    if (persist_env && pf <= PF_FEW) return launch_persist<DT, NT, EXACT, PF_FEW>(ctx, qkv, out, items, T, heads, st, ql, lds);
    return launch_pair<DT, NT, EXACT>(ctx, qkv, out, items, T, heads, st, ql, lds);
}

// NT = key tiles of 16 (13 for 197 tokens, 37 for 577).  EXACT: T > 16*(NT-1), so only the last tile has masked keys
// and the mask is resolved at compile time for every other tile.  CAUSAL: the text tower's mask (attend_tile).
template <int DT, int NT, bool EXACT, int OCC, bool CAUSAL = false>
__global__ void __launch_bounds__(256, OCC)
    attention_kernel(const uint16_t *__restrict__ qkv, uint16_t *__restrict__ ctx_out, int T, int heads, int qt_lim) {
    using E = vm_elem<DT>;
    using vec8 = typename E::vec8;
    constexpr int KROWS = NT * 16;
    constexpr int VROWS = KROWS;             // an odd last 16-key half step re-reads valid rows against P = 0
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *kl = smem;                         // [KROWS][128 B]
    char *vl = smem + (size_t)KROWS * 128;   // [VROWS][128 B]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, h = lane >> 4;
    const int b = blockIdx.x / heads, head = blockIdx.x - b * heads;
    const int H = heads * 64;
    // head-major input: block (part * heads + head) is a contiguous [M, 64] matrix, part 0 = q, 1 = k, 2 = v
    const size_t M = (size_t)(gridDim.x / heads) * T;
    auto block = [&](int part) { return qkv + ((size_t)(part * heads + head) * M + (size_t)b * T) * 64; };

    // ---- stage K and V rows by LDS-DMA (global_load_lds_dwordx4: 1 KiB = 8 rows per wave instruction) -----------
    // The swizzle is applied on the per-lane SOURCE chunk; rows past T re-read row T-1 (finite data: their scores
    // are masked to -inf and their probabilities are exactly 0), so nothing has to be zero-filled.
    auto load_q = [&](int qt, vec8 &q0, vec8 &q1) {
        int qtok = qt * 16 + r16;
        if (qtok > T - 1) qtok = T - 1;
        const uint16_t *qp = block(0) + (size_t)qtok * 64;
        q0 = __builtin_bit_cast(vec8, *reinterpret_cast<const uint4 *>(qp + 8 * h));
        q1 = __builtin_bit_cast(vec8, *reinterpret_cast<const uint4 *>(qp + 32 + 8 * h));
    };
    vec8 q0, q1;
    load_q(wave, q0, q1);  // first query tile of this wave: in flight together with the K/V rows
    {
        constexpr int GROUPS = (KROWS + VROWS) / 8;
        const int srow = lane >> 3, scp = lane & 7;
#pragma unroll
        for (int gi = 0; gi < (GROUPS + 3) / 4; ++gi) {
            const int grp = gi * 4 + wave;
            if (grp < GROUPS) {
                const int r = grp * 8 + srow;  // LDS row; K rows first, V rows behind them
                const bool is_v = r >= KROWS;
                int key = is_v ? r - KROWS : r;
                if (key > T - 1) key = T - 1;
                const uint16_t *src = block(is_v ? 2 : 1) + (size_t)key * 64 + ((scp ^ (r & 7)) << 3);
                __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(smem + grp * 1024), 16, 0, 0);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();

    for (int qt = wave; qt < qt_lim; qt += 4) {
        const int qtok = qt * 16 + r16;
        const bool qvalid = qtok < T;
        const vec8 qa = q0, qb = q1;
        if (qt + 4 < qt_lim) load_q(qt + 4, q0, q1);  // next tile's queries: their latency hides behind this tile

        attend_tile<DT, NT, EXACT, CAUSAL>(kl, vl, qa, qb, T, lane, qvalid,
                                           ctx_out + ((size_t)b * T + (qvalid ? qtok : 0)) * H + head * 64, 0, qtok);
    }
}

// Streaming variant for short sequences (two Q/K/V images fit in LDS: NT <= 13): one persistent workgroup per CU walks
// (frame, head) items.  Eight waves compute item i out of one LDS image while a ninth wave, the loader, fills the other
// image with item i+1 by LDS-DMA.  The plain kernel above alternates a pure load phase with a pure compute phase per
// workgroup, and the co-resident workgroups of a CU fall into step, so its time is load + compute; here it is
// max(load, compute).  One raw s_barrier per item; the compute waves issue no global loads at all (the queries come
// through LDS too), so they never wait on the vector-memory counter and their context stores drain in the background.
// (The loader is a wave of its own because vmcnt is per wave: the compiler guards every transposing LDS read with
// vmcnt(0) while an LDS-DMA of the same wave is in flight, which would serialise the two.)
template <int DT, int NT, bool EXACT, int CW>  // CW compute waves + 1 loader wave
__global__ void __launch_bounds__((CW + 1) * 64, 1)
    attention_stream_kernel(const uint16_t *__restrict__ qkv, uint16_t *__restrict__ ctx_out, int T, int heads,
                            int items, int qt_lim, int ctx_nt) {  // qt_lim: query tiles (of 16 rows) to compute per item, <= NT
    using E = vm_elem<DT>;
    using vec8 = typename E::vec8;
    constexpr int ROWS = NT * 16;
    constexpr int IMG = 3 * ROWS * 128;   // K rows, V rows, Q rows
    constexpr int QT = (NT + CW - 1) / CW;  // query tiles per compute wave
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = heads * 64;
    if (blockIdx.x >= items) return;

    if (wave == CW) {  // ---- loader ---------------------------------------------------------------------------
        // per-lane constants: a wave instruction covers 8 rows x 128 B; lane -> (row srow, stored chunk scp), and
        // since every group starts at a multiple of 8 rows the source chunk (scp ^ row & 7) is fixed per lane
        const int srow = lane >> 3, scp = lane & 7;
        const unsigned lane_off = (unsigned)((scp ^ srow) << 4);
        const size_t M = (size_t)(items / heads) * T;  // rows of each head-major [M, 64] block
        const int tmax = T - 1;
        int buf = 0;
        for (int item = blockIdx.x; item < items; item += gridDim.x, buf ^= 1) {
            const int b = item / heads, head = item - b * heads;
#pragma unroll
            for (int part = 0; part < 3; ++part) {  // LDS image order K, V, Q; qkv block order q, k, v
                const char *pbase = reinterpret_cast<const char *>(
                    qkv + ((size_t)((part == 2 ? 0 : part + 1) * heads + head) * M + (size_t)b * T) * 64);  // uniform
#pragma unroll
                for (int g = 0; g < ROWS / 8; ++g) {
                    if (part == 2 && g >= 2 * qt_lim) break;  // query rows nobody asked for are not fetched
                    int key = g * 8 + srow;
                    if (!EXACT || g * 8 + 7 >= 16 * (NT - 1)) key = key > tmax ? tmax : key;  // groups that can pass T
                    const unsigned off = (unsigned)key * 128 + lane_off;  // 8 rows = one contiguous KiB
                    __builtin_amdgcn_global_load_lds((gbl_ptr_t)(pbase + off),
                                                     (lds_ptr_t)(smem + buf * IMG + (part * (ROWS / 8) + g) * 1024), 16,
                                                     0, 2);  // aux 2 = nt: every Q/K/V byte is read exactly once
                                                             // (3.42 -> 3.34 ms per 880 frames)
                    // at most 28 KiB of this wave's fills queued in the CU's in-order memory pipe: the compute
                    // waves' context stores enter the same queue and must not wait behind a whole image
                    if ((g & 3) == 3) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            asm volatile("s_barrier" ::: "memory");
        }
        return;
    }

    // ---- compute waves ----------------------------------------------------------------------------------------
    const int r16 = lane & 15, h = lane >> 4;
    int buf = 0;
    for (int item = blockIdx.x; item < items; item += gridDim.x, buf ^= 1) {
        asm volatile("s_barrier" ::: "memory");  // the loader has landed this item's image
        const char *kl = smem + buf * IMG, *vl = kl + ROWS * 128, *ql = vl + ROWS * 128;
        const int b = item / heads, head = item - b * heads;
#pragma unroll
        for (int u = 0; u < QT; ++u) {
            const int qt = wave + CW * u;
            if (qt < qt_lim) {
                const int qtok = qt * 16 + r16;
                const bool qvalid = qtok < T;
                const vec8 qa = *reinterpret_cast<const vec8 *>(ql + qtok * 128 + ((h ^ (qtok & 7)) << 4));
                const vec8 qb = *reinterpret_cast<const vec8 *>(ql + qtok * 128 + (((h + 4) ^ (qtok & 7)) << 4));
                attend_tile<DT, NT, EXACT>(kl, vl, qa, qb, T, lane, qvalid,
                                           ctx_out + ((size_t)b * T + (qvalid ? qtok : 0)) * H + head * 64, ctx_nt);
            }
        }
    }
}

// 13 compute waves (one query tile each, four waves per SIMD at <= 128 registers) + the loader.  (Eight compute waves
// with up to two tiles each, 168 registers, were the first shape: DESIGN.md 4.3.  CW stays a template parameter of the
// kernel, whose QT loop is written for any count.)
template <int DT, int NT, bool EXACT>
int launch_stream(vm_ctx *ctx, const uint16_t *qkv, uint16_t *out, int B, int T, int heads, hipStream_t st, int qt_lim) {
    constexpr int CW = 13;
    const size_t lds = (size_t)NT * 16 * 128 * 6;
    auto kern = attention_stream_kernel<DT, NT, EXACT, CW>;
    if (int r = vm_lds_opt_in(ctx, kern, lds, "vm_attention")) return r;
    const int items = B * heads;
    const int grid = items < ctx->num_cus ? items : ctx->num_cus;
    vm_prof_scope prof(ctx, VM_PROF_ATTENTION, st);
    static const int ctx_nt_env = (int)VM_DEV_ENV("ATTN_CTX_NT", 1);   // context stores non-temporal (266 MB per launch, read
    // next by the projection GEMM long after L2 has turned over): 2.83 -> 2.77 ms per 880-frame step, three alternating pairs
    kern<<<grid, (CW + 1) * 64, lds, st>>>(qkv, out, T, heads, items, qt_lim < NT ? qt_lim : NT, ctx_nt_env);
    VM_LAUNCH_CHECK(ctx);
    return VM_OK;
}

template <int DT, int NT, bool EXACT, int OCC = (NT <= 13 ? 2 : 1), bool CAUSAL = false>
int launch(vm_ctx *ctx, const uint16_t *qkv, uint16_t *out, int B, int T, int heads, hipStream_t st, int qt_lim) {
    const size_t lds = (size_t)NT * 16 * 128 * 2;
    auto kern = attention_kernel<DT, NT, EXACT, OCC, CAUSAL>;
    if (int r = vm_lds_opt_in(ctx, kern, lds, "vm_attention")) return r;
    vm_prof_scope prof(ctx, VM_PROF_ATTENTION, st);
    kern<<<B * heads, 256, lds, st>>>(qkv, out, T, heads, qt_lim < NT ? qt_lim : NT);
    VM_LAUNCH_CHECK(ctx);
    return VM_OK;
}

template <int DT>
int dispatch(vm_ctx *ctx, const uint16_t *qkv, uint16_t *out, int B, int T, int heads, hipStream_t st, int q_rows,
             int causal) {
    const int nt = (T + 15) / 16;
    if (causal) {   // text tower (77 tokens): ONE build for every T <= 80, so a row's result cannot depend on T
        if (nt > 5) return vm_fail(ctx, VM_ERR_UNSUPPORTED, "causal attention: %d tokens > 80", T);
        return launch<DT, 5, false, 2, true>(ctx, qkv, out, B, T, heads, st, 5);
    }
    const int ql = q_rows > 0 ? (q_rows + 15) / 16 : nt;  // query tiles wanted (clamped to the kernel's NT at launch)
    if (nt == 13) {  // ViT-B/16-224: 197 tokens
        return launch_stream<DT, 13, true>(ctx, qkv, out, B, T, heads, st, ql);
    }
    if (nt == 37) return launch_long<DT, 37, true>(ctx, qkv, out, B, T, heads, st, ql);   // CLIP-L/14-336: 577 tokens
    if (nt <= 2) return launch<DT, 2, false>(ctx, qkv, out, B, T, heads, st, ql);
    if (nt <= 5) return launch<DT, 5, false>(ctx, qkv, out, B, T, heads, st, ql);
    if (nt <= 13) return launch<DT, 13, false>(ctx, qkv, out, B, T, heads, st, ql);
    if (nt <= 37) return launch_long<DT, 37, false>(ctx, qkv, out, B, T, heads, st, ql);
    return vm_fail(ctx, VM_ERR_UNSUPPORTED, "attention: %d tokens > 592", T);
}

}  // namespace

int vm_attention(vm_ctx *ctx, int dtype, const uint16_t *qkv, uint16_t *ctx_out, int B, int T, int heads,
                 hipStream_t st, int q_rows, int causal) {
    return dtype == VM_F16 ? dispatch<VM_F16>(ctx, qkv, ctx_out, B, T, heads, st, q_rows, causal)
                           : dispatch<VM_BF16>(ctx, qkv, ctx_out, B, T, heads, st, q_rows, causal);
}
