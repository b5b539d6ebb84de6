// The selection stage and the host scaffolding of the two-stage, certified searches that keep one fp32 key per
// (query, item): the grouped search (topk_group.hip, item = group) and the scoped search (topk_scope.hip, item = row).
// Defined here once: the order-preserving key images, the block-wide k-th key, "the best `take` of a
// compacted list" and the gap certificate of the finalize kernels; for the host the shared geometry, the workspace
// layout, the argument check and the dtype dispatch.  The reference arithmetic itself is topk_common.h's.
#pragma once
#include "topk_common.h"
#include "vm_internal.h"

#include <type_traits>

// order-preserving unsigned image of an fp32 score (bigger key = bigger value; -0 folded into +0; every image is > 0,
// so 0 is below every score's key)
__device__ __forceinline__ uint32_t okey32(float s) {
    uint32_t u = __float_as_uint(s);
    if (s == 0.f) u = 0;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dekey32(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// 64-bit composite key << 32 | ~index (bigger = better, unique): ties at one key go to the lower index
__device__ __forceinline__ unsigned long long composite(uint32_t key, int i) {
    return ((unsigned long long)key << 32) | (unsigned long long)(0xffffffffu - (uint32_t)i);
}

// largest T with at least `need` of the block's values >= T (PER values per thread, NT threads; every thread calls
// it): a bitwise search, one block-wide count per bit.  low_bit > 0 stops the search there: the result has its low
// bits clear and is a lower bound of the exact value (still at least `need` values >= T)
template <int NT, int PER>
__device__ __forceinline__ uint32_t block_kth_u32(const uint32_t (&v)[PER], int need, int low_bit = 0) {
    __shared__ int wsum[NT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t T = 0;
    for (int bit = 31; bit >= low_bit; --bit) {
        const uint32_t c = T | (1u << bit);
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) cnt += v[j] >= c ? 1 : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
        if (lane == 0) wsum[wave] = cnt;
        __syncthreads();
        int tot = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) tot += wsum[w];
        __syncthreads();
        if (tot >= need) T = c;
    }
    return T;
}

// The best `take` composites of list[0, cnt), cnt <= CAP and take <= min(cnt, CMAX), by one block of NT threads (all
// call it): the take-th largest key, then ties at that key by index.  Exactly take entries go to out_i / out_k, in
// any order (the finalize ranks them).
template <int NT, int CAP, int CMAX>
__device__ __forceinline__ void select_best(const unsigned long long *__restrict__ list, int cnt, int take,
                                            int *__restrict__ out_i, uint32_t *__restrict__ out_k) {
    constexpr int PER = CAP / NT;
    __shared__ int red[2][NT / 64];
    __shared__ int npos;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t hi[PER], lo[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = j * NT + tid;
        const unsigned long long c = i < cnt ? list[i] : 0ull;
        hi[j] = (uint32_t)(c >> 32);
        lo[j] = (uint32_t)c;  // ~index: bigger = lower index
    }
    const uint32_t T = block_kth_u32<NT>(hi, take);
    int above = 0, equal = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        above += hi[j] > T ? 1 : 0;
        equal += hi[j] == T ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        above += __shfl_xor(above, off, 64);
        equal += __shfl_xor(equal, off, 64);
    }
    if (lane == 0) {
        red[0][wave] = above;
        red[1][wave] = equal;
    }
    if (tid == 0) npos = 0;
    __syncthreads();
    above = equal = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        above += red[0][w];
        equal += red[1][w];
    }
    const int need_eq = take - above;
    uint32_t lo_cut = 0;  // keep the need_eq lowest indices among the keys == T
    if (need_eq < equal) {
        uint32_t le[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) le[j] = hi[j] == T ? lo[j] : 0u;
        lo_cut = block_kth_u32<NT>(le, need_eq);  // uniform branch: every thread sees the same counts
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        // an entry past cnt is no candidate even when T is 0 (take == 0); a position past CMAX is never written
        const bool keep = hi[j] > T || (hi[j] == T && lo[j] >= lo_cut && j * NT + tid < cnt);
        if (keep) {
            const int pos = atomicAdd(&npos, 1);
            if (pos < CMAX) {
                out_i[pos] = (int)(0xffffffffu - lo[j]);
                out_k[pos] = hi[j];
            }
        }
    }
}

// The gap certificate: the exact k-th score e is provably the k-th when it is strictly above the best
// fp32 score that was not re-scored (its key: rejected_key) / ||q|| + cert_eps(D)
__device__ __forceinline__ bool clears_gap(double e, uint32_t rejected_key, double qn, int D) {
    const double reject = (double)dekey32(rejected_key) / qn + cert_eps(D);
    return e > reject;
}

// ---- host --------------------------------------------------------------------------------------------------
// workspace bump allocator: every array starts 256-byte aligned
struct WsBump {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t at = off;
        off += vm_align_up(bytes, 256);
        return at;
    }
};

// The grid of a tile scan (topk_tile_scan.h): grid x = row blocks of scan_threads / 64 waves, one 16-row tile per wave
// and step, at most 8 blocks per CU; grid y = query groups of qt 16-query tiles.  `tiles` is the caller's own count of
// 16-row tiles of the capacity.
struct ScanGeom {
    int qt;       // 16-query tiles per scan block
    int qgroups;  // scan grid y
    int nbx;      // scan grid x
};
inline ScanGeom vm_scan_geom(const vm_memory *m, int Q, int64_t tiles, int scan_threads) {
    ScanGeom g;
    g.qt = Q <= 16 ? 1 : 2;
    g.qgroups = (Q + 16 * g.qt - 1) / (16 * g.qt);
    const int64_t nbx = (tiles + scan_threads / 64 - 1) / (scan_threads / 64);
    const int64_t lim = (int64_t)m->ctx->num_cus * 8;
    g.nbx = (int)(nbx < lim ? (nbx < 1 ? 1 : nbx) : lim);
    return g;
}

// the geometry the grouped and the scoped search share
struct TopkGeom : ScanGeom {
    int M;           // candidates re-scored exactly per query; the (M + 1)-th bounds the rest
    int nblk;        // redo row blocks
    int cmp_slices;  // compaction grid x
};
inline TopkGeom vm_topk_geom(const vm_memory *m, int Q, int k, int scan_threads, int redo_chunk) {
    TopkGeom g;
    static_cast<ScanGeom &>(g) = vm_scan_geom(m, Q, (m->cap + 15) / 16, scan_threads);
    g.M = k + (k / 4 > 8 ? k / 4 : 8);  // slack: near-ties between rank k and rank M are certified by the gap
    g.nblk = vm_topk_redo_blocks(m, redo_chunk);
    const int64_t sl = (m->cap + 8191) / 8192;
    g.cmp_slices = (int)(sl < 1 ? 1 : (sl > 64 ? 64 : sl));
    return g;
}

// The argument check of the grouped and scoped entry points.  missing: null, or the kind of memory the call needs and
// m is not; args_ok: the caller's own pointer and count tests; k_code: the error code of a k outside [1, kmax];
// need: the plan's workspace total.
inline int vm_topk_check(vm_memory *m, const char *missing, bool args_ok, const void *queries, int k, int kmax,
                         int k_code, int score_mode, const void *workspace, size_t workspace_bytes, size_t need,
                         const char *who) {
    vm_ctx *ctx = m->ctx;
    if (missing) return vm_fail(ctx, VM_ERR_INVALID, "%s: the memory is not %s", who, missing);
    if (!args_ok) return vm_fail(ctx, VM_ERR_INVALID, "%s: bad arguments", who);
    if (k < 1 || k > kmax)
        return k_code == VM_ERR_UNSUPPORTED ? vm_fail(ctx, k_code, "%s: k=%d > %d", who, k, kmax)
                                            : vm_fail(ctx, k_code, "%s: k=%d outside [1, %d]", who, k, kmax);
    if (int rc = vm_check_score_mode(ctx, score_mode)) return rc;
    if (!workspace || workspace_bytes < need)
        return vm_fail(ctx, VM_ERR_NOMEM, "%s: workspace %zu < %zu", who, workspace_bytes, need);
    if (((uintptr_t)workspace & 255) || ((uintptr_t)queries & 15))
        return vm_fail(ctx, VM_ERR_INVALID, "%s: workspace must be 256-byte and queries 16-byte aligned", who);
    return VM_OK;
}

// f(std::integral_constant<int, VM_F16 or VM_BF16>) for the memory's dtype
template <typename F>
inline int vm_by_dtype(const vm_memory *m, F f) {
    if (m->dtype == VM_F16) return f(std::integral_constant<int, VM_F16>());
    return f(std::integral_constant<int, VM_BF16>());
}
