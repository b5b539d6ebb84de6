// Group summaries: one centroid row and one key frame per group of a grouped memory (include/vidmem.h
// vm_memory_summaries).  The reference stores one embedding per chunk and searches those
// (src/components/neo4j_handler.py:229-242, src/pipeline/retriever_hybrid.py:293-306); a group's normalised mean is that
// vector, and the stored frame closest to it is the frame to show for the group.
//
// Live groups are numbered in row order by G(r) = ordinal[r] - ordinal[lo]: the ordinal column rises by 0 or 1 from one
// row id to the next (vm_internal.h), so group indices and first rows need no prefix scan.  The WINDOW is the groups
// g0 .. g1 - 1, g0 = max(*first_group, 0), g1 = min(g0 + max_groups, n_groups); window slot j holds group g0 + j.
//   bounds : one thread per age order.  A row that opens a group writes that group's first row (age order into the
//            workspace, row id and key into the outputs); the newest row writes the end of the last group and the
//            count; the blocks share the padding of every output.  first[j] .. first[j + 1] are the rows of slot j.
//   sum    : the hot pass, every row of the window once.  Lanes own 8 columns (one 16-byte load per row), a workgroup
//            of D / 8 lanes owns a run of consecutive groups and streams their rows in row order, 8 rows' loads in
//            flight ahead of the dependent fp64 adds - also across a group's end, so 16-row groups leave no bubble.
//            At a group's end: S_j^2 into LDS, one wave sums them left to right (the order is part of the contract),
//            then every lane divides and rounds its 8 columns once (round16.h) and stores 16 bytes.
//   score  : one exact pair per row - the row against the centroid of its group - on the events link kernel's LDS
//            streaming (events.hip): the block's 256 rows come slice by slice through two LDS buffers; the centroid
//            slice comes straight from global memory, where the lanes of one group read the same 16 bytes (a few lines
//            per wave instruction, cache hits after the group's first row).  The lane also sums the centroid's squares:
//            a second, independent fp64 chain beside the dot's.  Scores go to the workspace by age order.
//   select : one wave per window slot: arg-best of its scores by (score desc, row asc).
// No atomics, no workgroup waits for another; every launch reads the row count and *first_group on the device and is
// sized from the capacity and max_groups.
//
// A group's rows are summed by ONE workgroup in row order; nothing is split across workers, so the bits do not depend on
// the launch geometry.  The price: a single very long group streams through one workgroup.
#include "round16.h"
#include "topk_common.h"
#include "vm_internal.h"

#include <climits>

namespace {

constexpr int SM_CHUNK = 256;        // age orders per block of the bounds and score launches
constexpr int SM_AHEAD = 8;          // rows in flight per lane of the sum kernel
constexpr int SM_MAX_D = 8192;       // the sum kernel's workgroup is D / 8 lanes, at most 1,024
constexpr size_t SM_HEADER_BYTES = 256;

// The window of a call, from the device-side row count, the ordinal column and *first_group.
struct SmWindow {
    RingView rv;
    int64_t n_groups;  // live groups
    int64_t g0;        // first group of the window (may be >= n_groups)
    int64_t w;         // groups in the window: min(g0 + max_groups, n_groups) - g0, or 0
    int64_t ord0;      // ordinal of the oldest live row
};
__device__ __forceinline__ SmWindow sm_window(const int64_t *d_total, int64_t cap, int ring,
                                              const int64_t *__restrict__ gord, const int64_t *first_group,
                                              int64_t max_groups) {
    SmWindow s;
    s.rv = ring_view(*d_total, cap, ring);
    s.n_groups = 0;
    s.ord0 = 0;
    // group_view (vm_internal.h) written out: it reads the oldest row's slot as rv.head, and with that every kernel of
    // this file compiles to other instructions than the measured ones
    if (s.rv.n > 0) {
        s.ord0 = gord[slot_of(s.rv, 0)];
        s.n_groups = gord[slot_of(s.rv, s.rv.n - 1)] - s.ord0 + 1;
    }
    int64_t g0 = first_group ? *first_group : 0;
    s.g0 = g0 < 0 ? 0 : g0;
    int64_t w = s.n_groups - s.g0;
    if (w > max_groups) w = max_groups;
    s.w = w < 0 ? 0 : w;
    return s;
}

template <int DT>
__device__ __forceinline__ uint16_t sm_round16(double x) {
    return DT == VM_F16 ? vm_round16_f16(x) : vm_round16_bf16(x);
}

// ---- bounds ----------------------------------------------------------------------------------------------------------
// first[j], j in [0, w]: the age order of the first row of window slot j; first[w] = the end of slot w - 1 (the first
// row of group g1, or n).  An empty memory writes the count and nothing else.
__global__ void __launch_bounds__(SM_CHUNK)
    summary_bounds_kernel(const int64_t *__restrict__ d_total, int64_t cap, int ring, int D,
                          const int64_t *__restrict__ gkey, const int64_t *__restrict__ gord,
                          const int64_t *__restrict__ first_group, int64_t max_groups, int64_t *__restrict__ first,
                          uint16_t *__restrict__ out_cent, int64_t *__restrict__ out_first_rows,
                          int64_t *__restrict__ out_n_rows, int64_t *__restrict__ out_keys,
                          int64_t *__restrict__ out_key_rows, double *__restrict__ out_key_scores,
                          int64_t *__restrict__ out_n_groups) {
    const SmWindow win = sm_window(d_total, cap, ring, gord, first_group, max_groups);
    const int64_t n = win.rv.n;
    if (n == 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) *out_n_groups = 0;
        return;
    }
    // the padding of slots [w, max_groups), shared by the blocks
    const int64_t step = (int64_t)gridDim.x * SM_CHUNK, t0 = (int64_t)blockIdx.x * SM_CHUNK + threadIdx.x;
    for (int64_t i = win.w + t0; i < max_groups; i += step) {
        if (out_first_rows) out_first_rows[i] = -1;
        if (out_n_rows) out_n_rows[i] = -1;
        if (out_keys) out_keys[i] = -1;
        if (out_key_rows) out_key_rows[i] = -1;
        if (out_key_scores) out_key_scores[i] = 0.0;
    }
    if (out_cent) {
        uint4 *z = reinterpret_cast<uint4 *>(out_cent + (size_t)win.w * D);
        const int64_t pieces = (max_groups - win.w) * (D / 8);
        for (int64_t i = t0; i < pieces; i += step) z[i] = make_uint4(0, 0, 0, 0);
    }
    const int64_t o = t0;
    if (o >= n) return;
    const int64_t slot = slot_of(win.rv, o);
    const int64_t ord = gord[slot];
    const int64_t j = ord - win.ord0 - win.g0;
    if ((o == 0 || gord[slot_of(win.rv, o - 1)] != ord) && j >= 0 && j <= max_groups) {
        first[j] = o;  // j == max_groups: the end of the last slot
        if (j < max_groups) {
            if (out_first_rows) out_first_rows[j] = win.rv.base + o;
            if (out_keys) out_keys[j] = gkey[slot];
        }
    }
    if (o == n - 1) {
        if (j + 1 >= 0 && j + 1 <= max_groups) first[j + 1] = n;  // no group opens there: nobody else writes it
        *out_n_groups = win.n_groups;
    }
}

// ---- sum and normalise -------------------------------------------------------------------------------------------------
// Block b owns the window slots [b per, (b + 1) per), per = ceil(w / gridDim.x): consecutive groups, so consecutive
// rows.  blockDim.x = D / 8 rounded up to a whole wave; lane t owns the columns [8 t, 8 t + 8).  cent == nullptr: only
// the row counts are wanted, no row is read.  Dynamic LDS: 2 (D + 1) doubles.
template <int DT>
__global__ void __launch_bounds__(1024)
    summary_sum_kernel(const uint16_t *__restrict__ rows, const int64_t *__restrict__ gord,
                       const int64_t *__restrict__ d_total, int64_t cap, int ring, int D,
                       const int64_t *__restrict__ first_group, int64_t max_groups, const int64_t *__restrict__ first,
                       uint16_t *__restrict__ cent, int64_t *__restrict__ out_n_rows) {
    using E = vm_elem<DT>;
    extern __shared__ __attribute__((aligned(16))) double sm_sq[];  // [D] squares, [D] the norm, [D + 2 ..] the sums
    const SmWindow win = sm_window(d_total, cap, ring, gord, first_group, max_groups);
    if (win.w == 0) return;
    const int64_t per = (win.w + gridDim.x - 1) / gridDim.x;
    const int64_t j0 = (int64_t)blockIdx.x * per;
    const int64_t j1 = j0 + per < win.w ? j0 + per : win.w;
    if (j0 >= j1) return;  // block-uniform
    const int tid = threadIdx.x;
    if (out_n_rows)
        for (int64_t j = j0 + tid; j < j1; j += blockDim.x) out_n_rows[j] = first[j + 1] - first[j];
    if (!cent) return;
    const bool active = tid < D / 8;
    const int64_t r_end = first[j1];
    int64_t r = first[j0];
    // the lane's 16 bytes of the row of age order o, clamped into the block's rows; the lanes beyond D / 8 of the last
    // wave read the last piece again and drop it, so that no load sits under a branch
    const int piece = active ? tid : D / 8 - 1;
    auto load = [&](int64_t o) {
        const int64_t oc = o < r_end ? o : r_end - 1;
        return *(reinterpret_cast<const uint4 *>(rows + (size_t)slot_of(win.rv, oc) * D) + piece);
    };
    double S[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) S[k] = 0.0;
    double *sm_s = sm_sq + D + 2;  // [D] the sums, for the rolled divide loop
    int64_t j = j0, e = first[j0 + 1];  // the group being summed ends before age order e
    // Group j is complete (block-uniform): N, divide, round once, store.  Inlined once per row of a tile, so the loops
    // over the lane's 8 columns are rolled and read the sums back from LDS.
    auto finish = [&]() {
        if (active) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                sm_sq[tid * 8 + k] = __dmul_rn(S[k], S[k]);
                sm_s[tid * 8 + k] = S[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) S[k] = 0.0;
        __syncthreads();
        if (tid < 64) {  // one wave, every lane the same chain: left to right, one rounding per partial sum
            double acc = 0.0;
#pragma unroll 8
            for (int i = 0; i < D; ++i) acc = __dadd_rn(acc, sm_sq[i]);
            if (tid == 0) sm_sq[D] = __dsqrt_rn(acc);
        }
        __syncthreads();
        const double N = sm_sq[D];
        if (active) {
            uint64_t lo = 0, hi = 0;
#pragma unroll 1
            for (int k = 0; k < 8; ++k) {
                const uint64_t c = N == 0.0 ? 0 : sm_round16<DT>(__ddiv_rn(sm_s[tid * 8 + k], N));
                if (k < 4) lo |= c << (16 * k);
                else hi |= c << (16 * (k - 4));
            }
            *(reinterpret_cast<uint4 *>(cent + (size_t)j * D) + tid) =
                make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
        }
        ++j;
        e = j < j1 ? first[j + 1] : LLONG_MAX;
    };
    uint4 buf[SM_AHEAD], cur[SM_AHEAD];
#pragma unroll
    for (int u = 0; u < SM_AHEAD; ++u) buf[u] = load(r + u);
    while (r < r_end) {
#pragma unroll
        for (int u = 0; u < SM_AHEAD; ++u) cur[u] = buf[u];
        if (r + SM_AHEAD < r_end) {  // the next rows: in flight while these are summed
#pragma unroll
            for (int u = 0; u < SM_AHEAD; ++u) buf[u] = load(r + SM_AHEAD + u);
        }
#pragma unroll
        for (int u = 0; u < SM_AHEAD; ++u) {
            if (r + u < r_end) {  // block-uniform
                const uint16_t *xe = reinterpret_cast<const uint16_t *>(&cur[u]);
#pragma unroll
                for (int k = 0; k < 8; ++k) S[k] = __dadd_rn(S[k], E::to_double(xe[k]));
                if (r + u + 1 == e) finish();
            }
        }
        r += SM_AHEAD;
    }
}

// ---- score, the simple form -----------------------------------------------------------------------------------------
// Every lane runs ref_dot and ref_sumsq on global memory.  Kept as the yardstick of the streamed form and compiled into
// the developer library only (vm_common.h, VM_DEV_ENV): VIDMEM_SUMMARY_SIMPLE=1 in libvidmem_dev.so,
// tools/summary_probe.py.
#ifdef VM_DEV_SWITCHES
template <int DT>
__global__ void __launch_bounds__(SM_CHUNK)
    summary_score_kernel(const uint16_t *__restrict__ rows, const double *__restrict__ norm64,
                         const int64_t *__restrict__ gord, const int64_t *__restrict__ d_total, int64_t cap, int ring,
                         int D, const int64_t *__restrict__ first_group, int64_t max_groups,
                         const int64_t *__restrict__ first, const uint16_t *__restrict__ cent,
                         double *__restrict__ scores) {
    const SmWindow win = sm_window(d_total, cap, ring, gord, first_group, max_groups);
    if (win.w == 0) return;
    const int64_t o = (int64_t)blockIdx.x * SM_CHUNK + threadIdx.x;
    if (o < first[0] || o >= first[win.w]) return;
    const int64_t slot = slot_of(win.rv, o);
    const uint16_t *c = cent + (size_t)(gord[slot] - win.ord0 - win.g0) * D;
    const double cn = __dsqrt_rn(ref_sumsq<DT>(c, D));
    scores[o] = ref_cosine(ref_dot<DT>(c, rows + (size_t)slot * D, D), cn, norm64[slot]);
}
#endif  // VM_DEV_SWITCHES

// ---- score, streamed through LDS -------------------------------------------------------------------------------------
// LDS row t of a buffer holds the slice of age order 256 c + t; lane t sums its own row against its group's centroid.
// The row pitch is events.hip's: 144 bytes = 9 slots of 16 bytes, an odd number, so the 16 lanes of a ds_read_b128
// group, which read 16 consecutive rows modulo 16, hit 16 different slots.
constexpr int SM_SLICE = 64;                  // elements per stage
constexpr int SM_PIECES = SM_SLICE / 8;       // 16-byte pieces per row and stage
constexpr int SM_PITCH = SM_SLICE * 2 + 16;   // bytes
constexpr int SM_BUF = SM_CHUNK * SM_PITCH;   // one buffer
static_assert((SM_PITCH / 16) % 2 == 1, "an odd number of 16-byte slots per LDS row");

template <int DT>
__global__ void __launch_bounds__(SM_CHUNK)
    summary_score_stream_kernel(const uint16_t *__restrict__ rows, const double *__restrict__ norm64,
                                const int64_t *__restrict__ gord, const int64_t *__restrict__ d_total, int64_t cap,
                                int ring, int D, const int64_t *__restrict__ first_group, int64_t max_groups,
                                const int64_t *__restrict__ first, const uint16_t *__restrict__ cent,
                                double *__restrict__ scores) {
    using E = vm_elem<DT>;
    extern __shared__ __attribute__((aligned(16))) char sm_lds[];  // 2 x SM_BUF
    const SmWindow win = sm_window(d_total, cap, ring, gord, first_group, max_groups);
    if (win.w == 0) return;
    const int64_t lo = first[0], hi = first[win.w];  // the window's rows, as age orders
    const int64_t c0 = (int64_t)blockIdx.x * SM_CHUNK;
    if (c0 >= hi || c0 + SM_CHUNK <= lo) return;  // block-uniform: no row of the window here
    const int tid = threadIdx.x;
    // this thread's share of a stage: piece tid % 8 of the rows tid / 8 + 32 u
    const int piece = tid % SM_PIECES, r0 = tid / SM_PIECES;
    const uint4 *src[SM_PIECES];
#pragma unroll
    for (int u = 0; u < SM_PIECES; ++u) {
        const int64_t o = c0 + r0 + (SM_CHUNK / SM_PIECES) * u;
        src[u] = (o >= lo && o < hi) ? reinterpret_cast<const uint4 *>(rows + (size_t)slot_of(win.rv, o) * D) + piece
                                     : nullptr;
    }
    const int64_t o = c0 + tid;
    const bool mine = o >= lo && o < hi;
    const int64_t slot = mine ? slot_of(win.rv, o) : 0;
    const uint4 *csrc = mine ? reinterpret_cast<const uint4 *>(cent + (size_t)(gord[slot] - win.ord0 - win.g0) * D)
                             : nullptr;
    uint4 st[SM_PIECES], cq[SM_PIECES], cnext[SM_PIECES];
    auto load = [&](int s) {
#pragma unroll
        for (int u = 0; u < SM_PIECES; ++u) st[u] = src[u] ? src[u][s * SM_PIECES] : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int k = 0; k < SM_PIECES; ++k) cnext[k] = csrc ? csrc[s * SM_PIECES + k] : make_uint4(0, 0, 0, 0);
    };
    auto store = [&](int buf) {
        char *base = sm_lds + buf * SM_BUF;
#pragma unroll
        for (int u = 0; u < SM_PIECES; ++u)
            *reinterpret_cast<uint4 *>(base + (r0 + (SM_CHUNK / SM_PIECES) * u) * SM_PITCH + piece * 16) = st[u];
    };
    const int nsl = D / SM_SLICE;
    load(0);
    store(0);
    __syncthreads();
    double dot = 0.0, cc = 0.0;
    for (int s = 0; s < nsl; ++s) {
#pragma unroll
        for (int k = 0; k < SM_PIECES; ++k) cq[k] = cnext[k];
        if (s + 1 < nsl) load(s + 1);  // in flight while this slice is summed
        const char *pb = sm_lds + (s & 1) * SM_BUF + tid * SM_PITCH;
#pragma unroll
        for (int k = 0; k < SM_PIECES; ++k) {
            const uint4 b4 = *reinterpret_cast<const uint4 *>(pb + 16 * k);
            const uint16_t *ae = reinterpret_cast<const uint16_t *>(&cq[k]);
            const uint16_t *be = reinterpret_cast<const uint16_t *>(&b4);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const double a = E::to_double(ae[i]);
                dot = __dadd_rn(dot, __dmul_rn(a, E::to_double(be[i])));
                cc = __dadd_rn(cc, __dmul_rn(a, a));
            }
        }
        if (s + 1 < nsl) store((s + 1) & 1);  // last read two iterations ago, before the previous barrier
        __syncthreads();
    }
    if (mine) scores[o] = ref_cosine(dot, __dsqrt_rn(cc), norm64[slot]);
}

// ---- select ----------------------------------------------------------------------------------------------------------
// One wave per window slot: the best of scores[first[j], first[j + 1]) by (score desc, age order asc).
__global__ void __launch_bounds__(SM_CHUNK)
    summary_select_kernel(const int64_t *__restrict__ gord, const int64_t *__restrict__ d_total, int64_t cap, int ring,
                          const int64_t *__restrict__ first_group, int64_t max_groups,
                          const int64_t *__restrict__ first, const double *__restrict__ scores,
                          int64_t *__restrict__ out_key_rows, double *__restrict__ out_key_scores) {
    const SmWindow win = sm_window(d_total, cap, ring, gord, first_group, max_groups);
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (SM_CHUNK / 64);
    for (int64_t j = (int64_t)blockIdx.x * (SM_CHUNK / 64) + (threadIdx.x >> 6); j < win.w; j += waves) {
        const int64_t a = first[j], e = first[j + 1];
        double bs = 0.0;
        int64_t bo = -1;
        for (int64_t o = a + lane; o < e; o += 64) {  // ascending o: a later equal score does not replace
            const double v = scores[o];
            if (bo < 0 || v > bs) {
                bs = v;
                bo = o;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double s2 = __shfl_xor(bs, off, 64);
            const int64_t o2 = __shfl_xor(bo, off, 64);
            if (o2 >= 0 && (bo < 0 || s2 > bs || (s2 == bs && o2 < bo))) {
                bs = s2;
                bo = o2;
            }
        }
        if (lane == 0) {
            if (out_key_rows) out_key_rows[j] = win.rv.base + bo;
            if (out_key_scores) out_key_scores[j] = bs;
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------
struct SmPlan {
    int64_t slots;  // window slots the workspace holds: min(max_groups, capacity)
    unsigned nch;   // 256-row chunks of the capacity
    size_t off_first, off_scores, off_cent, total;
};

SmPlan summary_plan(const vm_memory *m, int64_t max_groups) {
    SmPlan p;
    p.slots = max_groups < m->cap ? max_groups : m->cap;
    if (p.slots < 0) p.slots = 0;
    const int64_t cap_pad = (m->cap + SM_CHUNK - 1) / SM_CHUNK * SM_CHUNK;
    p.nch = (unsigned)(cap_pad / SM_CHUNK);
    size_t off = SM_HEADER_BYTES;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += vm_align_up(bytes, 256);
        return at;
    };
    p.off_first = take((size_t)(p.slots + 1) * 8);
    p.off_scores = take((size_t)cap_pad * 8);
    p.off_cent = take((size_t)p.slots * m->D * 2);
    p.total = off;
    return p;
}

template <int DT>
int summary_run(vm_memory *m, const int64_t *first_group, int64_t max_groups, uint16_t *out_cent,
                int64_t *out_first_rows, int64_t *out_n_rows, int64_t *out_keys, int64_t *out_key_rows,
                double *out_key_scores, int64_t *out_n_groups, char *ws, hipStream_t st) {
    vm_ctx *ctx = m->ctx;
    const SmPlan p = summary_plan(m, max_groups);
    int64_t *first = (int64_t *)(ws + p.off_first);
    double *scores = (double *)(ws + p.off_scores);
    vm_prof_scope prof(ctx, VM_PROF_TOPK_EXACT, st);
    summary_bounds_kernel<<<p.nch, SM_CHUNK, 0, st>>>(m->d_total, m->cap, m->ring, m->D, m->gkey, m->gord, first_group,
                                                     max_groups, first, out_cent, out_first_rows, out_n_rows, out_keys,
                                                     out_key_rows, out_key_scores, out_n_groups);
    VM_LAUNCH_CHECK(ctx);
    if (max_groups == 0) return VM_OK;
    const bool keys = out_key_rows || out_key_scores;
    uint16_t *cent = out_cent ? out_cent : (keys ? (uint16_t *)(ws + p.off_cent) : nullptr);
    if (cent || out_n_rows) {
        const int nt = (m->D / 8 + 63) / 64 * 64;
        const int64_t most = (int64_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) * 8;
        const unsigned grid = (unsigned)(p.slots < most ? p.slots : most);
        auto kern = summary_sum_kernel<DT>;
        const size_t lds = (size_t)(m->D + 1) * 16;
        if (int rc = vm_lds_opt_in(ctx, kern, lds, "vm_memory_summaries")) return rc;
        kern<<<grid, nt, lds, st>>>(m->rows, m->gord, m->d_total, m->cap, m->ring, m->D, first_group, max_groups, first,
                                   cent, out_n_rows);
        VM_LAUNCH_CHECK(ctx);
    }
    if (!keys) return VM_OK;  // no second pass over the rows
#ifdef VM_DEV_SWITCHES
    if (VM_DEV_ENV("SUMMARY_SIMPLE", 0)) {
        summary_score_kernel<DT><<<p.nch, SM_CHUNK, 0, st>>>(m->rows, m->norm64, m->gord, m->d_total, m->cap, m->ring,
                                                            m->D, first_group, max_groups, first, cent, scores);
    } else
#endif
    {
        auto kern = summary_score_stream_kernel<DT>;
        if (int rc = vm_lds_opt_in(ctx, kern, 2 * SM_BUF, "vm_memory_summaries")) return rc;
        kern<<<p.nch, SM_CHUNK, 2 * SM_BUF, st>>>(m->rows, m->norm64, m->gord, m->d_total, m->cap, m->ring, m->D,
                                                 first_group, max_groups, first, cent, scores);
    }
    VM_LAUNCH_CHECK(ctx);
    const int64_t most = (int64_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) * 8;
    const int64_t want = (p.slots + SM_CHUNK / 64 - 1) / (SM_CHUNK / 64);
    summary_select_kernel<<<(unsigned)(want < most ? want : most), SM_CHUNK, 0, st>>>(
        m->gord, m->d_total, m->cap, m->ring, first_group, max_groups, first, scores, out_key_rows, out_key_scores);
    VM_LAUNCH_CHECK(ctx);
    return VM_OK;
}

}  // namespace

extern "C" size_t vm_memory_summaries_workspace_bytes(const vm_memory *m, int64_t max_groups) {
    if (!m) return 0;
    return summary_plan(m, max_groups).total;
}

extern "C" int vm_memory_summaries(vm_memory *m, const int64_t *first_group, int64_t max_groups, void *out_centroids,
                                   int64_t *out_first_rows, int64_t *out_n_rows, int64_t *out_keys,
                                   int64_t *out_key_rows, double *out_key_scores, int64_t *out_n_groups,
                                   void *workspace, size_t workspace_bytes, void *stream) {
    if (!m) return VM_ERR_INVALID;
    if (!m->gkey) return vm_fail(m->ctx, VM_ERR_INVALID, "vm_memory_summaries: the memory is not grouped");
    if (max_groups < 0 || !out_n_groups) return vm_fail(m->ctx, VM_ERR_INVALID, "vm_memory_summaries: bad arguments");
    if (m->D > SM_MAX_D)
        return vm_fail(m->ctx, VM_ERR_UNSUPPORTED, "vm_memory_summaries: D %d above %d", m->D, SM_MAX_D);
    const size_t need = summary_plan(m, max_groups).total;
    if (!workspace || workspace_bytes < need)
        return vm_fail(m->ctx, VM_ERR_NOMEM, "vm_memory_summaries: workspace %zu < %zu", workspace_bytes, need);
    if ((uintptr_t)workspace & 255)
        return vm_fail(m->ctx, VM_ERR_INVALID, "vm_memory_summaries: workspace must be 256-byte aligned");
    if (m->dtype == VM_F16)
        return summary_run<VM_F16>(m, first_group, max_groups, (uint16_t *)out_centroids, out_first_rows, out_n_rows,
                                   out_keys, out_key_rows, out_key_scores, out_n_groups, (char *)workspace,
                                   (hipStream_t)stream);
    return summary_run<VM_BF16>(m, first_group, max_groups, (uint16_t *)out_centroids, out_first_rows, out_n_rows,
                                out_keys, out_key_rows, out_key_scores, out_n_groups, (char *)workspace,
                                (hipStream_t)stream);
}
