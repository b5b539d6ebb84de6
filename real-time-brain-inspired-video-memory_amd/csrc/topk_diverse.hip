// Diverse cosine top-k: maximal marginal relevance (MMR) on the device (include/vidmem.h vm_topk_cosine_diverse).  The k
// answers of a query are picked greedily from an exact POOL of its best rows, each pick paying for its resemblance to what
// was picked before it: v_i = lam * e_i - (1 - lam) * max over the picked s of sim(i, s), with e the reference cosine of
// query and row and sim the reference cosine BETWEEN two stored rows.
//
// Three stages, the first of which is an existing search:
//   pool   : vm_topk_cosine_masked (a mask was given) or vm_topk_cosine_span with the open span (none was) with k = pool,
//            writing local row ids and fp64 cosines into the workspace: the shared driver of topk_scope_select.h - scan,
//            select, finalize, certificate, redo - under MaskScan / MaskScope or SpanScan / RowSpan, as it is.  The
//            `_exact` entry calls their `_exact` forms (key_image_exact)
//   pairs  : diverse_pair_kernel: S[q][i][j] = sim(pool row i, pool row j), fp64, both triangles.  One block per (query,
//            pair of 16-row pool tiles i <= j), one pair per thread: every chain of D products is sequential by
//            definition (topk_common.h ref_dot), the parallelism is the pairs
//   greedy : diverse_greedy_kernel: one wave per query, lane i owns pool entry i; k steps of one wave-wide arg-best on
//            (v desc, row id asc) and one coalesced read of the winner's row of S
// Every launch reads the row count from the device and is sized from the arguments: no allocation, no synchronisation, no
// host read-back - capturable.
#include "topk_scope_select.h"  // vm_key_image_plan: the pool search's workspace

namespace {

constexpr int DV_POOL = 64;       // pool entries per query = lanes of the greedy wave
constexpr int DV_TILE = 16;       // pool rows per pair tile
constexpr int DV_THREADS = 256;   // pairs: DV_TILE x DV_TILE
constexpr size_t DV_LDS_MAX = 160 * 1024;  // one tile of rows, 32 D bytes, must fit the LDS of a CU

// ---- the open span ------------------------------------------------------------------------------------------
__global__ void diverse_span_kernel(int64_t *__restrict__ lo, int64_t *__restrict__ hi, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        lo[i] = INT64_MIN;
        hi[i] = INT64_MAX;
    }
}

// ---- pairs ---------------------------------------------------------------------------------------------------
// grid (Q, tile pairs ti <= tj), DV_THREADS threads; dynamic LDS: tile ti's 16 rows [16][D].  Thread (ia, jb) scores pool
// entries i = 16 ti + ia and j = 16 tj + jb: row i from LDS, row j from global memory, the product of the two stored
// norms.  Products and the norm product commute, so sim(i, j) == sim(j, i) bit for bit and an off-diagonal block writes
// its value to both triangles.  An entry that is padding (row -1, or at and past `pool`) gives 0.0.  S: [Q][64][64].
template <int DT>
__global__ void __launch_bounds__(DV_THREADS)
    diverse_pair_kernel(const uint16_t *__restrict__ mem, const double *__restrict__ norm64,
                        const int64_t *__restrict__ d_total, int64_t cap, int ring, int D, int pool,
                        const int64_t *__restrict__ prow, double *__restrict__ S) {
    extern __shared__ __attribute__((aligned(16))) char dp_dyn[];
    uint16_t *tl = reinterpret_cast<uint16_t *>(dp_dyn);  // [DV_TILE][D]
    const int q = blockIdx.x, tid = threadIdx.x;
    const int T = (pool + DV_TILE - 1) / DV_TILE;
    int ti = 0, tj = blockIdx.y;  // pair number -> (ti, tj), rows of the upper triangle one after another
    while (tj >= T - ti) {
        tj -= T - ti;
        ++ti;
    }
    tj += ti;
    const RingView rv = ring_view(*d_total, cap, ring);
    // physical slot of pool entry idx, -1 for padding (a row id that is not live cannot come out of the pool stage)
    auto slot_at = [&](int idx) -> int64_t {
        if (idx >= pool) return -1;
        const int64_t r = prow[(size_t)q * pool + idx];
        const int64_t o = r - rv.base;
        return (r < 0 || o < 0 || o >= rv.n) ? -1 : slot_of(rv, o);
    };
    const int chunks = D / 8;
    for (int r = 0; r < DV_TILE; ++r) {  // the slot is uniform
        const int64_t p = slot_at(DV_TILE * ti + r);
        for (int c = tid; c < chunks; c += DV_THREADS)
            reinterpret_cast<uint4 *>(tl + (size_t)r * D)[c] =
                p >= 0 ? reinterpret_cast<const uint4 *>(mem + (size_t)p * D)[c] : make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    const int ia = tid / DV_TILE, jb = tid % DV_TILE;
    const int i = DV_TILE * ti + ia, j = DV_TILE * tj + jb;  // both below DV_POOL
    const int64_t pi = slot_at(i), pj = slot_at(j);
    double v = 0.0;
    if (pi >= 0 && pj >= 0)
        v = ref_cosine(ref_dot<DT>(tl + (size_t)ia * D, mem + (size_t)pj * D, D), norm64[pi], norm64[pj]);
    double *Sq = S + (size_t)q * DV_POOL * DV_POOL;
    Sq[i * DV_POOL + j] = v;
    if (ti != tj) Sq[j * DV_POOL + i] = v;
}

// ---- greedy --------------------------------------------------------------------------------------------------
// One wave per query.  Lane i holds pool entry i: its row id, its relevance e, whether it is still to be picked, and red =
// the largest sim to a picked row so far (plain >, from 0.0).  Step 0 takes the pool's first entry by definition; step t
// takes the largest v = lam e - (1 - lam) red, ties - -0.0 against +0.0 included - to the smaller row id.  The order is
// total over distinct row ids, so the butterfly leaves the same winner in every lane.  Output t: the winner's mapped row
// id, e and v; past the pool's entries -1 / 0.0 / 0.0.
__global__ void __launch_bounds__(64)
    diverse_greedy_kernel(const double *__restrict__ lam, int k, int pool, const int64_t *__restrict__ prow,
                          const double *__restrict__ pe, const double *__restrict__ S, int64_t row_stride,
                          int64_t row_offset, double *__restrict__ out_scores, int64_t *__restrict__ out_rows,
                          double *__restrict__ out_mmr) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const double l = lam[q], mu = __dsub_rn(1.0, l);
    const int64_t row = lane < pool ? prow[(size_t)q * pool + lane] : -1;
    const double e = lane < pool ? pe[(size_t)q * pool + lane] : 0.0;
    bool open = row >= 0;
    const unsigned long long entries = __ballot(open);
    const int np = __popcll(entries);
    const int first = np ? __ffsll(entries) - 1 : 0;
    const double *Sq = S + (size_t)q * DV_POOL * DV_POOL;
    double red = 0.0;
    for (int t = 0; t < k; ++t) {  // uniform
        const size_t at = (size_t)q * k + t;
        if (t >= np) {
            if (lane == 0) {
                out_rows[at] = -1;
                out_scores[at] = 0.0;
                out_mmr[at] = 0.0;
            }
            continue;
        }
        double bv = __dsub_rn(__dmul_rn(l, e), __dmul_rn(mu, red));
        int64_t br = open ? row : -1;  // -1: no candidate
        if (t == 0) br = lane == first ? row : -1;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double v2 = __shfl_xor(bv, off, 64);
            const int64_t r2 = __shfl_xor(br, off, 64);
            if (r2 >= 0 && (br < 0 || v2 > bv || (v2 == bv && r2 < br))) {
                bv = v2;
                br = r2;
            }
        }
        // the winner's pool entry; one lane: row ids differ.  No lane only when a NaN broke the order (undefined, but in bounds)
        const int hit = __ffsll(__ballot(open && row == br)) - 1;
        const int w = hit < 0 ? 0 : hit;
        const double ew = __shfl(e, w, 64);
        if (lane == w) open = false;
        if (lane < pool) {
            const double s = Sq[w * DV_POOL + lane];
            if (s > red) red = s;
        }
        if (lane == 0) {
            out_rows[at] = br * row_stride + row_offset;
            out_scores[at] = ew;
            out_mmr[at] = bv;
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------
// the pool search's workspace (topk_scope_select.h vm_key_image_plan for k = pool, the masked and the span search's alike;
// at offset 0), then the pool, the open span and S
struct DPlan {
    size_t pool_total, off_prow, off_pe, off_lo, off_hi, off_S, total;
};

DPlan diverse_plan(const vm_memory *m, int Q, int pool) {
    DPlan p;
    p.pool_total = vm_key_image_plan(m, Q, pool).total;
    WsBump ws;
    ws.off = vm_align_up(p.pool_total, 256);
    p.off_prow = ws.take((size_t)Q * pool * 8);
    p.off_pe = ws.take((size_t)Q * pool * 8);
    p.off_lo = ws.take((size_t)Q * 8);
    p.off_hi = ws.take((size_t)Q * 8);
    p.off_S = ws.take((size_t)Q * DV_POOL * DV_POOL * 8);
    p.total = ws.off;
    return p;
}

struct DiverseCall {
    const void *queries;
    int Q, k, pool;
    const double *lam;
    const uint32_t *masks;  // null: every live row
    int n_masks;
    const int32_t *mask_index;
    int use_min;
    double min_score;
    int64_t row_stride, row_offset;
    double *out_scores;
    int64_t *out_rows;
    double *out_mmr;
    int32_t *out_uncertified, *out_query_flags;  // null in the exhaustive-only entry point
    char *ws;
    size_t ws_bytes;
    hipStream_t stream;
};

constexpr int DV_Q_MAX = 1 << 20;  // the workspace offsets and Q * pool stay far inside 32 bits of queries

// Everything the call and the pool search inside it can refuse, before any launch
int diverse_check(vm_memory *m, const DiverseCall &c, const char *who) {
    vm_ctx *ctx = m->ctx;
    if (c.pool < 1 || c.pool > DV_POOL)
        return vm_fail(ctx, VM_ERR_INVALID, "%s: pool=%d outside [1, %d]", who, c.pool, DV_POOL);
    if (c.k < 1 || c.k > DV_POOL) return vm_fail(ctx, VM_ERR_INVALID, "%s: k=%d outside [1, %d]", who, c.k, DV_POOL);
    if (c.k > c.pool) return vm_fail(ctx, VM_ERR_INVALID, "%s: k=%d > pool=%d", who, c.k, c.pool);
    if (c.Q < 1 || c.Q > DV_Q_MAX) return vm_fail(ctx, VM_ERR_INVALID, "%s: Q=%d outside [1, %d]", who, c.Q, DV_Q_MAX);
    if (!c.queries || !c.lam) return vm_fail(ctx, VM_ERR_INVALID, "%s: null queries or lam", who);
    if (!c.out_scores || !c.out_rows || !c.out_mmr) return vm_fail(ctx, VM_ERR_INVALID, "%s: null outputs", who);
    if (c.row_stride < 1) return vm_fail(ctx, VM_ERR_INVALID, "%s: row_stride=%lld < 1", who, (long long)c.row_stride);
    if (c.masks)
        if (int rc = mask_operand_check(m, c.masks, c.n_masks, c.mask_index, c.Q, who)) return rc;
    if ((size_t)DV_TILE * m->D * 2 > DV_LDS_MAX)
        return vm_fail(ctx, VM_ERR_UNSUPPORTED, "%s: D=%d: a tile of %d rows does not fit the LDS", who, m->D, DV_TILE);
    const size_t need = diverse_plan(m, c.Q, c.pool).total;
    if (!c.ws || c.ws_bytes < need) return vm_fail(ctx, VM_ERR_NOMEM, "%s: workspace %zu < %zu", who, c.ws_bytes, need);
    if (((uintptr_t)c.ws & 255) || ((uintptr_t)c.queries & 15) || ((uintptr_t)c.lam & 7))
        return vm_fail(ctx, VM_ERR_INVALID, "%s: workspace must be 256-byte, queries 16-byte and lam 8-byte aligned",
                       who);
    return VM_OK;
}

// The pool: the masked or the open-span search with k = pool, raw scores, local row ids, into the workspace.  Profiled
// by the search itself under its own categories.
int diverse_pool(vm_memory *m, const DiverseCall &c, const DPlan &p, bool exact) {
    double *pe = (double *)(c.ws + p.off_pe);
    int64_t *prow = (int64_t *)(c.ws + p.off_prow);
    if (c.masks) {
        if (exact)
            return vm_topk_cosine_masked_exact(m, c.queries, c.Q, c.pool, c.masks, c.n_masks, c.mask_index, c.use_min,
                                               c.min_score, VM_SCORE_RAW, 1, 0, pe, prow, c.ws, p.pool_total, c.stream);
        return vm_topk_cosine_masked(m, c.queries, c.Q, c.pool, c.masks, c.n_masks, c.mask_index, c.use_min, c.min_score,
                                     VM_SCORE_RAW, 1, 0, pe, prow, c.out_uncertified, c.out_query_flags, c.ws,
                                     p.pool_total, c.stream);
    }
    int64_t *lo = (int64_t *)(c.ws + p.off_lo), *hi = (int64_t *)(c.ws + p.off_hi);
    diverse_span_kernel<<<(c.Q + 255) / 256, 256, 0, c.stream>>>(lo, hi, c.Q);
    VM_LAUNCH_CHECK(m->ctx);
    if (exact)
        return vm_topk_cosine_span_exact(m, c.queries, c.Q, c.pool, lo, hi, c.use_min, c.min_score, VM_SCORE_RAW, 1, 0, pe,
                                         prow, c.ws, p.pool_total, c.stream);
    return vm_topk_cosine_span(m, c.queries, c.Q, c.pool, lo, hi, c.use_min, c.min_score, VM_SCORE_RAW, 1, 0, pe, prow,
                               c.out_uncertified, c.out_query_flags, c.ws, p.pool_total, c.stream);
}

template <int DT>
int diverse_pick(vm_memory *m, const DiverseCall &c, const DPlan &p) {
    vm_prof_scope prof(m->ctx, VM_PROF_TOPK_FINALIZE, c.stream);
    const double *pe = (const double *)(c.ws + p.off_pe);
    const int64_t *prow = (const int64_t *)(c.ws + p.off_prow);
    double *S = (double *)(c.ws + p.off_S);
    const int T = (c.pool + DV_TILE - 1) / DV_TILE;
    const size_t lds = (size_t)DV_TILE * m->D * 2;
    auto kern = diverse_pair_kernel<DT>;
    // above what a launch gets without the attribute from D = 2,048 on
    if (int rc = vm_lds_opt_in(m->ctx, kern, lds, "vm_topk_cosine_diverse")) return rc;
    kern<<<dim3(c.Q, T * (T + 1) / 2), DV_THREADS, lds, c.stream>>>(m->rows, m->norm64, m->d_total, m->cap, m->ring,
                                                                    m->D, c.pool, prow, S);
    VM_LAUNCH_CHECK(m->ctx);
    diverse_greedy_kernel<<<c.Q, 64, 0, c.stream>>>(c.lam, c.k, c.pool, prow, pe, S, c.row_stride, c.row_offset,
                                                    c.out_scores, c.out_rows, c.out_mmr);
    VM_LAUNCH_CHECK(m->ctx);
    return VM_OK;
}

int diverse_entry(vm_memory *m, const DiverseCall &c, bool exact, const char *who) {
    if (!m) return VM_ERR_INVALID;
    if (int rc = diverse_check(m, c, who)) return rc;
    const DPlan p = diverse_plan(m, c.Q, c.pool);
    if (int rc = diverse_pool(m, c, p, exact)) return rc;
    return vm_by_dtype(m, [&](auto dt) { return diverse_pick<decltype(dt)::value>(m, c, p); });
}

}  // namespace

extern "C" size_t vm_topk_diverse_workspace_bytes(const vm_memory *m, int Q, int pool) {
    if (!m || Q < 1 || Q > DV_Q_MAX || pool < 1 || pool > DV_POOL) return 0;
    return diverse_plan(m, Q, pool).total;
}

extern "C" int vm_topk_cosine_diverse(vm_memory *m, const void *queries, int Q, int k, int pool, const double *lam,
                                      const uint32_t *masks, int n_masks, const int32_t *mask_index, int use_min_score,
                                      double min_score, int64_t row_stride, int64_t row_offset, double *out_scores,
                                      int64_t *out_rows, double *out_mmr, int32_t *out_uncertified,
                                      int32_t *out_query_flags, void *workspace, size_t workspace_bytes, void *stream) {
    const DiverseCall c = {queries,       Q,          k,          pool,       lam,      masks,   n_masks,
                           mask_index,    use_min_score, min_score, row_stride, row_offset, out_scores, out_rows,
                           out_mmr,       out_uncertified, out_query_flags, (char *)workspace, workspace_bytes,
                           (hipStream_t)stream};
    return diverse_entry(m, c, false, "vm_topk_cosine_diverse");
}

extern "C" int vm_topk_cosine_diverse_exact(vm_memory *m, const void *queries, int Q, int k, int pool, const double *lam,
                                            const uint32_t *masks, int n_masks, const int32_t *mask_index,
                                            int use_min_score, double min_score, int64_t row_stride, int64_t row_offset,
                                            double *out_scores, int64_t *out_rows, double *out_mmr, void *workspace,
                                            size_t workspace_bytes, void *stream) {
    const DiverseCall c = {queries,    Q,          k,         pool,       lam,        masks,      n_masks,
                           mask_index, use_min_score, min_score, row_stride, row_offset, out_scores, out_rows,
                           out_mmr,    nullptr,    nullptr,   (char *)workspace, workspace_bytes, (hipStream_t)stream};
    return diverse_entry(m, c, true, "vm_topk_cosine_diverse_exact");
}
