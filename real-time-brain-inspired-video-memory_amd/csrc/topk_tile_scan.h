// The fp32 MFMA tile scan of the grouped, scoped, masked and range searches, written once: every live row
// against a tile of queries, with the list scan's numerics - topk_scan_kernel's (topk.hip) instruction over the same
// operand layout, then x 1/||row|| - which is what cert_eps(D) (topk_common.h) is a statement about.  A search supplies
// a POLICY for what differs, defined next to the rest of that search (topk_group.hip, topk_scope.hip, range.hip,
// topk_mask.hip):
//   struct Args                      what the policy reads and writes, passed to the kernel by value
//   template <int QT> struct QState  per-query state of the block's QT * 16 queries in static LDS (empty: none)
//   struct View                      what the policy derives once per thread from the live-row view
//   load_query(qs, a, i, q, live)    thread i < QT * 16 fills entry i of qs for query q; !live: q is past Q
//   view(a, rv)
//   skip_tile<QT>(qs, a, l)          wave-uniform: true = no row of this tile is wanted; the policy has then written
//                                    what a skipped tile writes, and the tile's rows are not read
//   epilogue<QT>(qs, a, pv, l, s)    what becomes of the tile's scores s[t][j] = acc[t][j] / ||row p0 + j||
// The MFMA loop stays in the kernel body: as a function of its own it compiles to other code (4.1.2).
#pragma once
#include "topk_select.h"

#include <climits>
#include <type_traits>

constexpr int TS_THREADS = 256;

// where a lane stands in a tile: acc[t][j] = <row in slot p0() + j, query q0 + 16 t + r16>
struct TileLane {
    int64_t n, tile;  // live rows, tile
    int q0, Q, lane, r16, h;
    // the lane's first slot; p0 + 3 is below cap_pad (the columns are padded to 64 rows)
    __device__ __forceinline__ int64_t p0() const { return tile * 16 + 4 * h; }
};

// The 16 tags of a tile against the scopes of the block's queries, before any row data: lane (r16, h) tests row r16
// against queries 4h .. 4h+3 of each 16-query tile.  Wave-uniform: some (row, query) pair of the tile is in scope.
template <int QT>
__device__ __forceinline__ bool tile_in_scope(const int64_t *__restrict__ tag, const int64_t *slo, const int64_t *shi,
                                              const TileLane &l) {
    const int64_t trow = l.tile * 16 + l.r16;
    bool hit = false;
    if (trow < l.n) {
        const int64_t tg = tag[trow];
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int c = 0; c < 4; ++c) hit |= in_scope(tg, slo[16 * t + 4 * l.h + c], shi[16 * t + 4 * l.h + c]);
    }
    return __ballot(hit) != 0ull;
}

// The per-query state of a policy with tag scopes: the scopes of the block's QT * 16 queries.  16-byte aligned: the tag
// pre-test reads a lane's four scopes with two 16-byte LDS loads per array.  A policy with more per-query state derives.
template <int QT>
struct TagQState {
    alignas(16) int64_t lo[QT * 16], hi[QT * 16];
};
// entry i = the scope of query q; a query past Q (!live) has the empty scope
template <class QS>
__device__ __forceinline__ void load_tag_scope(QS &qs, const int64_t *lo, const int64_t *hi, int i, int q, bool live) {
    qs.lo[i] = live ? lo[q] : LLONG_MAX;
    qs.hi[i] = live ? hi[q] : LLONG_MIN;
}

// grid (row blocks, query groups of QT*16); dynamic LDS: the query tile, QT * 16 * D * 2 bytes.  16-row tiles in
// physical order, the row tile the A operand straight from global memory, the query tile the B operand from
// chunk-swizzled LDS, score = acc * rnorm32.
template <int DT, int QT, class P>
__global__ void __launch_bounds__(TS_THREADS)
    tile_scan_kernel(const uint16_t *__restrict__ mem, const float *__restrict__ rnorm,
                     const uint16_t *__restrict__ queries, const int64_t *__restrict__ d_total, int64_t cap, int ring,
                     int D, int Q, const typename P::Args a) {
    using E = vm_elem<DT>;
    using vec8 = typename E::vec8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint4 *qlds = reinterpret_cast<uint4 *>(smem);
    __shared__ typename P::template QState<QT> qs;
    const int chunks = D / 8;
    constexpr int nw = TS_THREADS / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, h = lane >> 4;
    const int q0 = blockIdx.y * (QT * 16);
    for (int idx = tid; idx < QT * 16 * chunks; idx += TS_THREADS) {
        const int q = idx / chunks, ci = idx - q * chunks;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (q0 + q < Q) v = reinterpret_cast<const uint4 *>(queries + (size_t)(q0 + q) * D)[ci];
        qlds[q * chunks + ((ci & ~15) | ((ci ^ q) & 15))] = v;
    }
    if (tid < QT * 16) P::load_query(qs, a, tid, q0 + tid, q0 + tid < Q);
    __syncthreads();
    const RingView rv = ring_view(*d_total, cap, ring);
    const typename P::View pv = P::view(a, rv);
    const int64_t n = rv.n;
    const int64_t ntiles = (n + 15) / 16;
    const int ksteps = D / 32;
    constexpr int LB = 8;
    const uint4 *qrow = qlds + r16 * chunks;
    const int tstride = 16 * chunks;
    const int64_t tile_step = (int64_t)gridDim.x * nw;
    for (int64_t tile = (int64_t)blockIdx.x * nw + wave; tile < ntiles; tile += tile_step) {
        const TileLane l = {n, tile, q0, Q, lane, r16, h};
        if (P::template skip_tile<QT>(qs, a, l)) continue;
        int64_t row = tile * 16 + r16;
        if (row > n - 1) row = n - 1;  // tail lanes re-read the last row; the policy masks their scores
        const uint4 *src = reinterpret_cast<const uint4 *>(mem + (size_t)row * D) + h;
        f32x4 acc[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int s0 = 0; s0 < ksteps; s0 += LB) {
            uint4 cur[LB];
#pragma unroll
            for (int u = 0; u < LB; ++u) cur[u] = src[(s0 + u < ksteps ? s0 + u : ksteps - 1) * 4];
#pragma unroll
            for (int u = 0; u < LB; ++u) {
                if (s0 + u < ksteps) {
                    const int ci = h + 4 * (s0 + u);
                    const vec8 av = __builtin_bit_cast(vec8, cur[u]);
                    const uint4 *qp = qrow + ((ci & ~15) | ((ci ^ r16) & 15));
#pragma unroll
                    for (int t = 0; t < QT; ++t) acc[t] = E::mfma16(av, __builtin_bit_cast(vec8, qp[t * tstride]), acc[t]);
                }
            }
        }
        const float4 rn = *reinterpret_cast<const float4 *>(rnorm + l.p0());
        const float rnv[4] = {rn.x, rn.y, rn.z, rn.w};
        // the policy gets the scores, not the accumulators: handed to a function, the accumulators themselves compile to
        // more registers (4.1.2)
        float s[QT][4];
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) s[t][j] = acc[t][j] * rnv[j];
        P::template epilogue<QT>(qs, a, pv, l, s);
    }
}

// The one launcher.  The kernel's LDS is the query tile (dynamic) plus the policy's per-query state (static); the
// context grants the dynamic part (vm_lds_opt_in).
template <int DT, int QT, class P>
int vm_tile_scan_qt(vm_memory *m, const ScanGeom &g, const void *queries, int Q, const typename P::Args &a,
                    hipStream_t st) {
    const size_t lds = (size_t)QT * 16 * m->D * 2;
    auto kern = tile_scan_kernel<DT, QT, P>;
    if (int rc = vm_lds_opt_in(m->ctx, kern, lds, "tile scan")) return rc;
    kern<<<dim3(g.nbx, g.qgroups), TS_THREADS, lds, st>>>(m->rows, m->rnorm32, (const uint16_t *)queries, m->d_total,
                                                         m->cap, m->ring, m->D, Q, a);
    VM_LAUNCH_CHECK(m->ctx);
    return VM_OK;
}
template <int DT, class P>
int vm_tile_scan(vm_memory *m, const ScanGeom &g, const void *queries, int Q, const typename P::Args &a,
                 hipStream_t st) {
    return g.qt == 1 ? vm_tile_scan_qt<DT, 1, P>(m, g, queries, Q, a, st)
                     : vm_tile_scan_qt<DT, 2, P>(m, g, queries, Q, a, st);
}
