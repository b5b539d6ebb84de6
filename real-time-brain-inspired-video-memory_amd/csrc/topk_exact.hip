// Exhaustive fp64 cosine: every (query, row) pair scored exactly as the reference does
// (src/components/pre_llm_injector.py:374-388: three left-to-right fp64 sums, sqrt, guards, one division),
// then a stable top-k.  Used (a) as the fallback for queries the fast scan cannot certify, (b) for the
// post-compression filter (src/pipeline/retriever_hybrid.py:494-504), (c) as an on-device checker.
// Also home of what the three redos share (vm_internal.h): the row-block count vm_topk_redo_blocks, the redo scan of rows
// vm_topk_redo_scan (the row redo here, topk_scope.hip, topk_mask.hip and topk_span.hip; the grouped one carries a group
// across chunks and is topk_group.hip's own) and the merge of the slice winners vm_topk_redo_merge (all three).
#include "topk_common.h"
#include "vm_internal.h"

namespace {

// grid (ceil(n/256), Q).  Thread = one stored row; the query sits in LDS.  `order_to_phys`: rows are addressed
// by age order o (0 = oldest) and mapped to the physical slot (o + head) % cap, so out[q, o] is in row-id order.
template <int DT>
__global__ void __launch_bounds__(256)
    cosine_exact_kernel(const uint16_t *__restrict__ queries, const uint16_t *__restrict__ rows, int64_t n,
                        int64_t head, int64_t cap, int D, double *__restrict__ out, int64_t out_stride) {
    using E = vm_elem<DT>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint16_t *ql = reinterpret_cast<uint16_t *>(smem);
    __shared__ double qnorm_sh;
    const int q = blockIdx.y;
    const uint16_t *qv = queries + (size_t)q * D;
    for (int i = threadIdx.x; i < D / 8; i += blockDim.x)
        reinterpret_cast<uint4 *>(ql)[i] = reinterpret_cast<const uint4 *>(qv)[i];
    __syncthreads();
    if (threadIdx.x == 0) qnorm_sh = __dsqrt_rn(ref_sumsq<DT>(ql, D));
    __syncthreads();
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n) return;
    const uint16_t *mv = rows + (size_t)slot_of(RingView{n, head, 0, cap}, o) * D;
    double dot = 0.0, nb = 0.0;
    for (int i = 0; i < D; i += 8) {
        const uint4 b = *reinterpret_cast<const uint4 *>(mv + i);
        const uint4 a = *reinterpret_cast<const uint4 *>(ql + i);
        const uint16_t *ae = reinterpret_cast<const uint16_t *>(&a);
        const uint16_t *be = reinterpret_cast<const uint16_t *>(&b);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double x = E::to_double(ae[j]), y = E::to_double(be[j]);
            dot = __dadd_rn(dot, __dmul_rn(x, y));
            nb = __dadd_rn(nb, __dmul_rn(y, y));
        }
    }
    out[(size_t)q * out_stride + o] = ref_cosine(dot, qnorm_sh, __dsqrt_rn(nb));
}

// fp32 operands (vm_cosine_exact, VM_F32): same arithmetic on the values as they are - every fp32 is exact in fp64.
// grid (ceil(n/256), Q); S is small here (the segments of a handful of hits), so the query stays in global memory.
__global__ void __launch_bounds__(256)
    cosine_exact_f32_kernel(const float *__restrict__ queries, const float *__restrict__ rows, int64_t n, int D,
                            double *__restrict__ out) {
    const int q = blockIdx.y;
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n) return;
    const float *qv = queries + (size_t)q * D, *mv = rows + (size_t)o * D;
    double dot = 0.0, na = 0.0, nb = 0.0;
    for (int i = 0; i < D; ++i) {
        const double x = (double)qv[i], y = (double)mv[i];
        dot = __dadd_rn(dot, __dmul_rn(x, y));
        na = __dadd_rn(na, __dmul_rn(x, x));
        nb = __dadd_rn(nb, __dmul_rn(y, y));
    }
    const double qn = __dsqrt_rn(na), mn = __dsqrt_rn(nb);
    out[(size_t)q * n + o] = ref_cosine(dot, qn, mn);
}

// One block per query: k rounds, each finds the best key strictly after the previous winner in
// (score desc, index asc) order.  Stateless, so any n works.  col_limit (may be null): query q sees only the first
// min(n, col_limit[q]) columns (vm_topk_select: the rows that existed before the query's own chunk was appended).
__global__ void __launch_bounds__(256)
    topk_select_kernel(const double *__restrict__ scores, int64_t n, int64_t stride, int k, int use_min,
                       double min_score, int score_mode, int64_t base, int64_t row_stride, int64_t row_offset,
                       double *__restrict__ out_scores, int64_t *__restrict__ out_rows,
                       const int64_t *__restrict__ col_limit) {
    __shared__ double ws[256];
    __shared__ int64_t wi[256];
    const int q = blockIdx.x, tid = threadIdx.x;
    const double *s = scores + (size_t)q * stride;
    if (col_limit) {
        const int64_t lim = col_limit[q];
        n = lim < 0 ? 0 : (lim < n ? lim : n);
    }
    double prev_s = INFINITY;
    int64_t prev_i = -1;
    for (int r = 0; r < k; ++r) {
        double bs = -INFINITY;
        int64_t bi = -1;
        for (int64_t i = tid; i < n; i += 256) {
            const double v = s[i];
            const bool after_prev = v < prev_s || (v == prev_s && i > prev_i);
            const bool beats = bi < 0 || v > bs || (v == bs && i < bi);
            if (after_prev && beats) {
                bs = v;
                bi = i;
            }
        }
        ws[tid] = bs;
        wi[tid] = bi;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if (tid < off) {
                const double s2 = ws[tid + off];
                const int64_t i2 = wi[tid + off];
                const bool take = i2 >= 0 && (wi[tid] < 0 || s2 > ws[tid] || (s2 == ws[tid] && i2 < wi[tid]));
                if (take) {
                    ws[tid] = s2;
                    wi[tid] = i2;
                }
            }
            __syncthreads();
        }
        prev_s = ws[0];
        prev_i = wi[0];
        __syncthreads();
        if (tid == 0) {
            double shown = prev_s;
            bool ok = prev_i >= 0;
            if (ok) {  // shown_score / passes_min (topk_common.h), written out: the helpers change this kernel
                if (score_mode == VM_SCORE_UNIT_INTERVAL) shown = __ddiv_rn(__dadd_rn(1.0, prev_s), 2.0);
                if (use_min && !(shown > min_score)) ok = false;
            }
            out_scores[(size_t)q * k + r] = ok ? shown : 0.0;
            out_rows[(size_t)q * k + r] = ok ? (base + prev_i) * row_stride + row_offset : -1;
        }
        if (prev_i < 0) {  // exhausted: pad the rest
            for (int r2 = r + 1 + tid; r2 < k; r2 += 256) {
                out_scores[(size_t)q * k + r2] = 0.0;
                out_rows[(size_t)q * k + r2] = -1;
            }
            break;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// Exhaustive redo of the queries the fast scan could not certify (vm_topk_cosine's out_query_flags).
// Both kernels read the row count from the DEVICE counter and take flags from device memory: no host read-back,
// no allocation, capturable into a hipGraph, and free (two near-empty launches) when no query is flagged.
// ---------------------------------------------------------------------------------------------------------
constexpr int REDO_THREADS = 256;
constexpr int REDO_KMAX = 64;

// grid = nblk row blocks; every block walks all Q flags and, for each flagged query, scores its contiguous slice of
// age orders exactly as the reference does (src/components/pre_llm_injector.py:374-388) and keeps the slice's
// stable top-k: part[(block * Q + q) * k + i] = {score fp64, age order int64}.  CHUNK scores are held in LDS per
// selection pass.  P = the row predicate (vm_internal.h).  NoScope: every live row, the scores sit in dynamic LDS behind
// the query.  A scoped P (TagScope, MaskScope, RowSpan): only the rows it admits are scored and may win, and a chunk with
// none costs its tags or mask words only (nothing under RowSpan); the scores and the in-scope marks sit in static LDS.
template <int DT, int CHUNK, class P>
__global__ void __launch_bounds__(REDO_THREADS)
    topk_redo_scan_kernel(const uint16_t *__restrict__ queries, const uint16_t *__restrict__ rows,
                          const double *__restrict__ norm64, const int64_t *__restrict__ d_total, int64_t cap, int ring,
                          int D, int Q, int k, const int32_t *__restrict__ flags, double *__restrict__ part_s,
                          int64_t *__restrict__ part_o, const P pred) {
    constexpr bool SCOPED = P::scoped;  // a predicate selects the rows
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint16_t *ql = reinterpret_cast<uint16_t *>(smem);  // [D]
    double *sc;                                         // [CHUNK]
    uint8_t *live = nullptr;                            // [CHUNK], SCOPED only: the row is in the query's scope
    if constexpr (SCOPED) {
        __shared__ double sc_sh[CHUNK];
        __shared__ uint8_t live_sh[CHUNK];
        sc = sc_sh;
        live = live_sh;
    } else {
        sc = reinterpret_cast<double *>(smem + (size_t)D * 2);
    }
    __shared__ double run_s[REDO_KMAX], new_s[REDO_KMAX], red_s[REDO_THREADS / 64];
    __shared__ int64_t run_o[REDO_KMAX], new_o[REDO_KMAX], red_o[REDO_THREADS / 64];
    __shared__ double qnorm_sh;
    const int tid = threadIdx.x;
    const RingView rv = ring_view(*d_total, cap, ring);
    const int64_t per = (rv.n + gridDim.x - 1) / gridDim.x;
    const int64_t lo = (int64_t)blockIdx.x * per;
    const int64_t hi = lo + per < rv.n ? lo + per : rv.n;
    // The common launch has no flagged query at all: find that out with independent strided loads and one block-wide OR
    // (the per-query test below is a chain of dependent scalar loads: 0.43 ms for the 7,040 queries an 8-GPU step
    // brings to every shard).
    int any = 0;
    for (int i = tid; i < Q; i += REDO_THREADS) any |= flags[i];
    if (!__syncthreads_or(any)) return;
    for (int q = 0; q < Q; ++q) {
        if (flags[q] == 0) continue;  // uniform
        __syncthreads();
        for (int i = tid; i < D / 8; i += REDO_THREADS)
            reinterpret_cast<uint4 *>(ql)[i] = reinterpret_cast<const uint4 *>(queries + (size_t)q * D)[i];
        if (tid < k) {
            run_s[tid] = -INFINITY;
            run_o[tid] = -1;
        }
        __syncthreads();
        if (tid == 0) qnorm_sh = __dsqrt_rn(ref_sumsq<DT>(ql, D));
        __syncthreads();
        const double qn = qnorm_sh;
        const typename P::Q pq = pred.at(q);
        for (int64_t c0 = lo; c0 < hi; c0 += CHUNK) {
            const int cn = (int)(hi - c0 < CHUNK ? hi - c0 : CHUNK);
            int mine = 0;
            for (int i = tid; i < cn; i += REDO_THREADS) {
                const int64_t p = slot_of(rv, c0 + i);
                bool in = true;
                if constexpr (SCOPED) {
                    in = pq.in(p);
                    live[i] = in ? 1 : 0;
                }
                if (in) {
                    // norm64: the reference's norm of the stored row, computed at append
                    sc[i] = ref_cosine(ref_dot<DT>(ql, rows + (size_t)p * D, D), qn, norm64[p]);
                    mine = 1;
                }
            }
            if constexpr (SCOPED) {
                if (!__syncthreads_or(mine)) continue;  // uniform: nothing of this chunk is in scope
            } else {
                __syncthreads();
            }
            // candidates = this chunk's scores followed by the running list
            block_select<REDO_THREADS>(cn + k, k,
                         [&](int i, double &v, int64_t &o) {
                             if (i < cn) {
                                 v = sc[i];
                                 o = c0 + i;
                                 if constexpr (SCOPED) o = live[i] ? o : -1;
                             } else {
                                 v = run_s[i - cn];
                                 o = run_o[i - cn];
                             }
                         },
                         new_s, new_o, red_s, red_o);
            if (tid < k) {
                run_s[tid] = new_s[tid];
                run_o[tid] = new_o[tid];
            }
            __syncthreads();
        }
        if (tid < k) {
            part_s[((size_t)blockIdx.x * Q + q) * k + tid] = run_s[tid];
            part_o[((size_t)blockIdx.x * Q + q) * k + tid] = run_o[tid];
        }
    }
}

// grid = Q; a block whose query is not flagged exits at once.  Stable top-k over the nblk * k slice winners,
// then the same output mapping as the fast path (score mode, min_score, global row id, -1 / 0.0 padding).  The one merge
// of the row, scoped and grouped redos; gkey / out_keys are the grouped search's (null otherwise).
__global__ void __launch_bounds__(REDO_THREADS)
    topk_redo_merge_kernel(const double *__restrict__ part_s, const int64_t *__restrict__ part_o, int nblk, int Q,
                           int k, const int32_t *__restrict__ flags, const int64_t *__restrict__ d_total,
                           int64_t cap, int ring, int use_min, double min_score, int score_mode,
                           int64_t row_stride, int64_t row_offset, double *__restrict__ out_scores,
                           int64_t *__restrict__ out_rows, const int64_t *__restrict__ gkey,
                           int64_t *__restrict__ out_keys) {
    __shared__ double win_s[REDO_KMAX], red_s[REDO_THREADS / 64];
    __shared__ int64_t win_o[REDO_KMAX], red_o[REDO_THREADS / 64];
    const int q = blockIdx.x, tid = threadIdx.x;
    if (flags[q] == 0) return;
    const RingView rv = ring_view(*d_total, cap, ring);
    block_select<REDO_THREADS>(nblk * k, k,
                 [&](int i, double &v, int64_t &o) {
                     const int b = i / k, e = i - b * k;
                     v = part_s[((size_t)b * Q + q) * k + e];
                     o = part_o[((size_t)b * Q + q) * k + e];
                 },
                 win_s, win_o, red_s, red_o);
    if (tid < k) {
        const int64_t o = win_o[tid];
        double shown = win_s[tid];
        bool ok = o >= 0;
        if (ok) {
            shown = shown_score(shown, score_mode);
            ok = passes_min(use_min, shown, min_score);
        }
        out_scores[(size_t)q * k + tid] = ok ? shown : 0.0;
        out_rows[(size_t)q * k + tid] = ok ? (rv.base + o) * row_stride + row_offset : -1;
        if (out_keys) out_keys[(size_t)q * k + tid] = ok ? gkey[slot_of(rv, o)] : -1;
    }
}

}  // namespace

int vm_topk_redo_blocks(const vm_memory *m, int chunk) {
    int64_t b = (m->cap + chunk - 1) / chunk;
    if (b > m->ctx->num_cus) b = m->ctx->num_cus;
    return b < 1 ? 1 : (int)b;
}

template <class P>
int vm_topk_redo_scan(vm_memory *m, const void *queries, int Q, int k, const P &pred, const int32_t *flags, int nblk,
                      double *part_s, int64_t *part_o, hipStream_t st) {
    constexpr int CHUNK = P::scoped ? VM_REDO_CHUNK_SCOPED : VM_REDO_CHUNK;
    // the unscoped scan keeps its scores in dynamic LDS behind the query, the scoped ones in static LDS
    const size_t lds = (size_t)m->D * 2 + (P::scoped ? 0 : (size_t)CHUNK * 8);
    auto launch = [&](auto kern) {
        kern<<<nblk, REDO_THREADS, lds, st>>>((const uint16_t *)queries, m->rows, m->norm64, m->d_total, m->cap, m->ring,
                                              m->D, Q, k, flags, part_s, part_o, pred);
    };
    if (m->dtype == VM_F16) launch(topk_redo_scan_kernel<VM_F16, CHUNK, P>);
    else launch(topk_redo_scan_kernel<VM_BF16, CHUNK, P>);
    VM_LAUNCH_CHECK(m->ctx);
    return VM_OK;
}
template int vm_topk_redo_scan(vm_memory *, const void *, int, int, const NoScope &, const int32_t *, int, double *,
                               int64_t *, hipStream_t);
template int vm_topk_redo_scan(vm_memory *, const void *, int, int, const TagScope &, const int32_t *, int, double *,
                               int64_t *, hipStream_t);
template int vm_topk_redo_scan(vm_memory *, const void *, int, int, const MaskScope &, const int32_t *, int, double *,
                               int64_t *, hipStream_t);
template int vm_topk_redo_scan(vm_memory *, const void *, int, int, const RowSpan &, const int32_t *, int, double *,
                               int64_t *, hipStream_t);

int vm_topk_redo_merge(vm_memory *m, const double *part_s, const int64_t *part_o, int nblk, int Q, int k,
                       const int32_t *flags, int use_min, double min_score, int score_mode, int64_t row_stride,
                       int64_t row_offset, double *out_scores, int64_t *out_rows, const int64_t *gkey,
                       int64_t *out_keys, hipStream_t st) {
    topk_redo_merge_kernel<<<Q, REDO_THREADS, 0, st>>>(part_s, part_o, nblk, Q, k, flags, m->d_total, m->cap, m->ring,
                                                      use_min, min_score, score_mode, row_stride, row_offset,
                                                      out_scores, out_rows, gkey, out_keys);
    VM_LAUNCH_CHECK(m->ctx);
    return VM_OK;
}

extern "C" int vm_cosine_exact(vm_ctx *ctx, const void *queries, int Q, const void *rows, int64_t S, int D,
                               int dtype, double *out, void *stream) {
    // S == 0: out [Q, 0] holds nothing, and an empty device tensor's address is null - neither rows nor out is needed
    if (!ctx || !queries || Q <= 0 || S < 0 || (S > 0 && (!rows || !out)))
        return vm_fail(ctx, VM_ERR_INVALID, "vm_cosine_exact: bad arguments");
    if (S == 0) return VM_OK;
    dim3 grid((unsigned)((S + 255) / 256), Q);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == VM_F32) {
        if (D <= 0) return vm_fail(ctx, VM_ERR_INVALID, "vm_cosine_exact: D=%d", D);
        cosine_exact_f32_kernel<<<grid, 256, 0, st>>>((const float *)queries, (const float *)rows, S, D, out);
        VM_LAUNCH_CHECK(ctx);
        return VM_OK;
    }
    if (D <= 0 || D % 8 != 0) return vm_fail(ctx, VM_ERR_UNSUPPORTED, "vm_cosine_exact: D=%d not a multiple of 8", D);
    if (dtype == VM_F16)
        cosine_exact_kernel<VM_F16><<<grid, 256, (size_t)D * 2, st>>>((const uint16_t *)queries,
                                                                     (const uint16_t *)rows, S, 0, S, D, out, S);
    else if (dtype == VM_BF16)
        cosine_exact_kernel<VM_BF16><<<grid, 256, (size_t)D * 2, st>>>((const uint16_t *)queries,
                                                                      (const uint16_t *)rows, S, 0, S, D, out, S);
    else
        return vm_fail(ctx, VM_ERR_INVALID, "bad dtype %d", dtype);
    VM_LAUNCH_CHECK(ctx);
    return VM_OK;
}

extern "C" size_t vm_topk_exact_workspace_bytes(const vm_memory *m, int Q, int k) {
    (void)k;
    if (!m || Q <= 0) return 0;
    return vm_align_up((size_t)Q * (size_t)m->cap * 8, 256);
}

extern "C" int vm_topk_cosine_exact(vm_memory *m, const void *queries, int Q, int k, int use_min_score,
                                    double min_score, int score_mode, int64_t row_stride, int64_t row_offset,
                                    double *out_scores, int64_t *out_rows, void *workspace,
                                    size_t workspace_bytes, void *stream) {
    if (!m) return VM_ERR_INVALID;
    vm_ctx *ctx = m->ctx;
    if (!queries || !out_scores || !out_rows || Q <= 0 || k <= 0)
        return vm_fail(ctx, VM_ERR_INVALID, "vm_topk_cosine_exact: bad arguments");
    // This entry point reads the HOST mirror of the row count (it sizes the grid), so it is not for graph replay.
    const int64_t total = m->h_total;
    int64_t n = total < m->cap ? total : m->cap, head = 0, base = 0;
    if (m->ring && total > m->cap) {
        head = total % m->cap;
        base = total - m->cap;
    }
    if (!workspace || workspace_bytes < (size_t)Q * (size_t)(n > 0 ? n : 1) * 8)
        return vm_fail(ctx, VM_ERR_NOMEM, "vm_topk_cosine_exact: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    vm_prof_scope prof(ctx, VM_PROF_TOPK_EXACT, st);
    double *sc = (double *)workspace;
    if (n > 0) {
        dim3 grid((unsigned)((n + 255) / 256), Q);
        if (m->dtype == VM_F16)
            cosine_exact_kernel<VM_F16><<<grid, 256, (size_t)m->D * 2, st>>>((const uint16_t *)queries, m->rows, n,
                                                                            head, m->cap, m->D, sc, n);
        else
            cosine_exact_kernel<VM_BF16><<<grid, 256, (size_t)m->D * 2, st>>>((const uint16_t *)queries, m->rows,
                                                                             n, head, m->cap, m->D, sc, n);
        VM_LAUNCH_CHECK(ctx);
    }
    topk_select_kernel<<<Q, 256, 0, st>>>(sc, n, n, k, use_min_score, min_score, score_mode, base, row_stride,
                                          row_offset, out_scores, out_rows, nullptr);
    VM_LAUNCH_CHECK(ctx);
    return VM_OK;
}

extern "C" int vm_topk_select(vm_ctx *ctx, const double *scores, int Q, int64_t S, const int64_t *col_limit, int k,
                              int64_t row_base, double *out_scores, int64_t *out_rows, void *stream) {
    if (!ctx || !scores || !out_scores || !out_rows || Q <= 0 || S < 0 || k <= 0)
        return vm_fail(ctx, VM_ERR_INVALID, "vm_topk_select: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    vm_prof_scope prof(ctx, VM_PROF_TOPK_EXACT, st);
    topk_select_kernel<<<Q, 256, 0, st>>>(scores, S, S, k, 0, 0.0, VM_SCORE_RAW, row_base, 1, 0, out_scores, out_rows,
                                          col_limit);
    VM_LAUNCH_CHECK(ctx);
    return VM_OK;
}

extern "C" size_t vm_topk_redo_workspace_bytes(const vm_memory *m, int Q, int k) {
    if (!m || Q <= 0 || k <= 0 || k > REDO_KMAX) return 0;
    return vm_align_up((size_t)vm_topk_redo_blocks(m, VM_REDO_CHUNK) * Q * k * 16, 256);
}

extern "C" int vm_topk_redo_flagged(vm_memory *m, const void *queries, int Q, int k, int use_min_score,
                                    double min_score, int score_mode, int64_t row_stride, int64_t row_offset,
                                    const int32_t *query_flags, double *out_scores, int64_t *out_rows,
                                    void *workspace, size_t workspace_bytes, void *stream) {
    if (!m) return VM_ERR_INVALID;
    vm_ctx *ctx = m->ctx;
    if (!queries || !out_scores || !out_rows || !query_flags || Q <= 0 || k <= 0)
        return vm_fail(ctx, VM_ERR_INVALID, "vm_topk_redo_flagged: bad arguments");
    if (k > REDO_KMAX) return vm_fail(ctx, VM_ERR_UNSUPPORTED, "vm_topk_redo_flagged: k=%d > %d", k, REDO_KMAX);
    if (int rc = vm_check_score_mode(ctx, score_mode)) return rc;
    const int nblk = vm_topk_redo_blocks(m, VM_REDO_CHUNK);
    const size_t need = (size_t)nblk * Q * k * 16;
    if (!workspace || workspace_bytes < need)
        return vm_fail(ctx, VM_ERR_NOMEM, "vm_topk_redo_flagged: workspace %zu < %zu", workspace_bytes, need);
    if (((uintptr_t)workspace & 15) || ((uintptr_t)queries & 15))
        return vm_fail(ctx, VM_ERR_INVALID, "vm_topk_redo_flagged: pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    vm_prof_scope prof(ctx, VM_PROF_TOPK_EXACT, st);
    double *part_s = (double *)workspace;
    int64_t *part_o = (int64_t *)((char *)workspace + (size_t)nblk * Q * k * 8);
    if (int rc = vm_topk_redo_scan(m, queries, Q, k, NoScope{}, query_flags, nblk, part_s, part_o, st)) return rc;
    return vm_topk_redo_merge(m, part_s, part_o, nblk, Q, k, query_flags, use_min_score, min_score, score_mode, row_stride,
                              row_offset, out_scores, out_rows, nullptr, nullptr, st);
}
