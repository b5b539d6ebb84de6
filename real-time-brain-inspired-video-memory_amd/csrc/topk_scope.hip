// Scoped cosine top-k: the k best rows among those whose int64 TAG lies in the query's inclusive range [lo, hi]
// (include/vidmem.h).  Replaces the per-graph predicate of the two scans the row search replaces
// (src/pipeline/retriever_hybrid.py:295 `MATCH (c:Chunk {graph_uuid: $graph_uuid})`,
// src/components/pre_llm_injector.py:395-396 `WHERE c.graph_uuid = $graph_uuid`): one memory holds many videos, a
// query names the video or the time window it wants.
//
// The row ranking is vm_topk_cosine's, taken over the in-scope rows only.  Same two-stage, certified design as topk.hip
// and topk_group.hip, with which it shares topk_select.h (key images, block-wide selection, gap
// certificate, plan scaffold, argument check) and topk_tile_scan.h (the scan; ScopeScan below is its policy); a row is a
// group of one whose fp32 key is 0 when it is out of scope:
//   scan     : per 16-row tile the wave first reads the tile's 16 tags and tests them against the scopes of its query
//              tile; a tile with no (row, query) pair in scope is skipped WITHOUT reading its rows (8 bytes per row
//              instead of 2 D) and only zeroes its keys.  Otherwise fp32 MFMA scores with the list scan's numerics (the
//              same instruction over the same operand layout, then x 1/||row||), the per-pair mask applied again, one
//              order-preserving key per (query, physical slot): F[q][slot], 0 = out of scope (below every score's key)
//   select   : per query the best M + 1 in-scope rows by (fp32 key desc, age order asc): a cut from a strided sample of
//              the keys, a parallel compaction of every in-scope row at or above it, a block-wide selection.  A query
//              with more than SEL_CAP rows at its cut is flagged VM_FLAG_OVERFLOW
//   finalize : the best M re-scored exactly (topk_common.h), ordered (score desc, row asc), filtered, k kept.  Certified
//              when the scope holds at most M rows, or when the exact k-th score clears the (M+1)-th IN-SCOPE fp32
//              score / ||q|| by cert_eps(D), strictly.  Out-of-scope rows have key 0 and never reach the certificate
//   redo     : flagged queries scored exhaustively over their in-scope rows, slices of age orders per block, stable
//              top-k per slice (vm_topk_redo_scan: the row redo's kernel with the tag predicate), then the one merge of
//              every redo (vm_topk_redo_merge; both topk_exact.hip).  Flags and
//              counts are read on the device; near-empty when nothing is flagged.
// Every launch reads the row count from the device and sizes its grid from the capacity: capturable.
#include "topk_scope_select.h"  // the select stage (cut, compaction, selection): shared with topk_clip.hip
#include "topk_tile_scan.h"

#include <climits>

namespace {

// ---- scan --------------------------------------------------------------------------------------------------
// The scoped policy of the tile scan (topk_tile_scan.h): four keys per lane, F[q * fstride + slot] = the order-preserving
// key of the fp32 score, or 0 when the row is out of the query's scope or past the live rows.
struct ScopeScan {
    struct Args {
        const int64_t *tag, *scope_lo, *scope_hi;
        int64_t fstride;
        uint32_t *F;
    };
    template <int QT>
    struct QState {  // 16-byte aligned: the tag pre-test reads a lane's four scopes with two 16-byte LDS loads per array
        alignas(16) int64_t lo[QT * 16], hi[QT * 16];
    };
    struct View {};
    template <class QS>
    static __device__ __forceinline__ void load_query(QS &qs, const Args &a, int i, int q, bool live) {
        qs.lo[i] = live ? a.scope_lo[q] : LLONG_MAX;  // queries past Q have the empty scope
        qs.hi[i] = live ? a.scope_hi[q] : LLONG_MIN;
    }
    static __device__ __forceinline__ View view(const Args &, const RingView &) { return {}; }
    template <int QT>
    static __device__ __forceinline__ bool skip_tile(const QState<QT> &qs, const Args &a, const TileLane &l) {
        if (tile_in_scope<QT>(a.tag, qs.lo, qs.hi, l)) return false;
#pragma unroll
        for (int t = 0; t < QT; ++t) {  // a skipped tile only zeroes its keys
            const int q = l.q0 + 16 * t + l.r16;
            if (q < l.Q) *reinterpret_cast<uint4 *>(a.F + (size_t)q * a.fstride + l.p0()) = make_uint4(0, 0, 0, 0);
        }
        return true;
    }
    template <int QT>
    static __device__ __forceinline__ void epilogue(const QState<QT> &qs, const Args &a, const View &,
                                                    const TileLane &l, const float (&s)[QT][4]) {
        int64_t tj[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) tj[j] = a.tag[l.p0() + j];
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const int q = l.q0 + 16 * t + l.r16;
            if (q >= l.Q) continue;
            const int64_t lo = qs.lo[16 * t + l.r16], hi = qs.hi[16 * t + l.r16];
            uint32_t key[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                key[j] = (l.p0() + j < l.n && in_scope(tj[j], lo, hi)) ? okey32(s[t][j]) : 0u;
            *reinterpret_cast<uint4 *>(a.F + (size_t)q * a.fstride + l.p0()) = make_uint4(key[0], key[1], key[2], key[3]);
        }
    }
};

// ---- finalize ----------------------------------------------------------------------------------------------
// One block per query.  Ranks the C candidates by (fp32 key desc, order asc): the first nc = min(C, M) are re-scored
// exactly, the (M+1)-th (if any) bounds every other in-scope row.
template <int DT>
__global__ void __launch_bounds__(SF_THREADS)
    scope_finalize_kernel(const uint16_t *__restrict__ mem, const double *__restrict__ norm64,
                          const uint16_t *__restrict__ queries, const int64_t *__restrict__ d_total, int64_t cap,
                          int ring, int D, const int *__restrict__ cand_o, const uint32_t *__restrict__ cand_k,
                          const int *__restrict__ cand_n, int M, int k, int use_min, double min_score, int score_mode,
                          int64_t row_stride, int64_t row_offset, double *__restrict__ out_scores,
                          int64_t *__restrict__ out_rows, int *__restrict__ uncertified, int *__restrict__ flags,
                          int *__restrict__ user_flags) {
    extern __shared__ __attribute__((aligned(16))) char sf_dyn[];
    uint16_t *ql = reinterpret_cast<uint16_t *>(sf_dyn);  // [D]
    __shared__ int so[SCMAX], lo_[SCMAX];
    __shared__ uint32_t sk[SCMAX], lk[SCMAX];
    __shared__ double es[SCMAX];
    __shared__ double qn_sh;
    __shared__ int flag_sh;
    const int q = blockIdx.x, tid = threadIdx.x;
    const RingView rv = ring_view(*d_total, cap, ring);
    const int C = cand_n[q];
    if (C < 0) {  // uniform: more rows at the cut than the buffer holds -> the exhaustive redo answers this query
        for (int i = tid; i < k; i += SF_THREADS) {
            out_scores[(size_t)q * k + i] = 0.0;
            out_rows[(size_t)q * k + i] = -1;
        }
        if (tid == 0) {
            flags[q] = VM_FLAG_OVERFLOW;
            if (user_flags) user_flags[q] = VM_FLAG_OVERFLOW;
            if (uncertified) atomicAdd(uncertified, 1);
        }
        return;
    }
    const int nc = C < M ? C : M;
    for (int i = tid; i < D / 8; i += SF_THREADS)
        reinterpret_cast<uint4 *>(ql)[i] = reinterpret_cast<const uint4 *>(queries + (size_t)q * D)[i];
    if (tid < C) {
        lo_[tid] = cand_o[(size_t)q * SCMAX + tid];
        lk[tid] = cand_k[(size_t)q * SCMAX + tid];
    }
    if (tid == 0) flag_sh = VM_FLAG_CERTIFIED;
    __syncthreads();
    if (tid < C) {  // rank by (fp32 key desc, order asc)
        const int o = lo_[tid];
        const uint32_t key = lk[tid];
        int r = 0;
        for (int j = 0; j < C; ++j) r += (lk[j] > key || (lk[j] == key && lo_[j] < o)) ? 1 : 0;
        so[r] = o;
        sk[r] = key;
    }
    if (tid == SF_THREADS - 1) qn_sh = __dsqrt_rn(ref_sumsq<DT>(ql, D));
    __syncthreads();
    const double qn = qn_sh;
    if (tid < nc) {
        const int64_t p = slot_of(rv, so[tid]);
        es[tid] = ref_cosine(ref_dot<DT>(ql, mem + (size_t)p * D, D), qn, norm64[p]);
    }
    __syncthreads();
    if (tid < nc) {
        const double e = es[tid];
        const int o = so[tid];
        int r = 0;
        for (int d = 0; d < nc; ++d) r += (es[d] > e || (es[d] == e && so[d] < o)) ? 1 : 0;
        if (r < k) {
            const double shown = shown_score(e, score_mode);
            const bool pass = passes_min(use_min, shown, min_score);
            out_scores[(size_t)q * k + r] = pass ? shown : 0.0;
            out_rows[(size_t)q * k + r] = pass ? (rv.base + o) * row_stride + row_offset : -1;
        }
        // certification: the exact k-th score against the best fp32 score of an in-scope row that was not re-scored
        const int kth = (k < nc ? k : nc) - 1;
        if (r == kth && C > M && qn != 0.0 && !clears_gap(e, sk[M], qn, D)) flag_sh = VM_FLAG_GAP;
    }
    for (int i = nc + tid; i < k; i += SF_THREADS) {
        out_scores[(size_t)q * k + i] = 0.0;
        out_rows[(size_t)q * k + i] = -1;
    }
    __syncthreads();
    if (tid == 0) {
        int f = flag_sh;
        // domain of the certificate (topk_common.h cert_eps; bf16 only): outside it the in-call redo answers the query
        if constexpr (DT == VM_BF16) {
            if (f == VM_FLAG_CERTIFIED && rv.n > 0 && (d_total[VM_GSTATE_OUTSIDE] != 0 || cert_norm_outside(qn)))
                f = VM_FLAG_GAP;
        }
        flags[q] = f;
        if (user_flags) user_flags[q] = f;
        if (f && uncertified) atomicAdd(uncertified, 1);
    }
}

// ---- redo --------------------------------------------------------------------------------------------------
__global__ void scope_fill_flags_kernel(int32_t *__restrict__ flags, int Q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Q) flags[i] = 1;
}

// ---- host --------------------------------------------------------------------------------------------------
struct SPlan : TopkGeom {
    int64_t fstride;
    size_t off_co, off_ck, off_cn, off_flags, off_cut, off_cc, off_cbuf, off_ps, off_po, total;
};

SPlan scope_plan(const vm_memory *m, int Q, int k) {
    SPlan p;
    static_cast<TopkGeom &>(p) = vm_topk_geom(m, Q, k, TS_THREADS, VM_REDO_CHUNK_SCOPED);
    p.fstride = (m->cap + 63) / 64 * 64;  // the columns' padding: a tail tile writes its 16 keys
    WsBump ws;
    ws.take((size_t)Q * (size_t)p.fstride * 4);  // F at offset 0: [Q][slot] fp32 keys
    p.off_co = ws.take((size_t)Q * SCMAX * 4);
    p.off_ck = ws.take((size_t)Q * SCMAX * 4);
    p.off_cn = ws.take((size_t)Q * 4);
    p.off_flags = ws.take((size_t)Q * 4);
    p.off_cut = ws.take((size_t)Q * 4);
    p.off_cc = ws.take((size_t)Q * 4);
    p.off_cbuf = ws.take((size_t)Q * SEL_CAP * 8);
    p.off_ps = ws.take((size_t)p.nblk * Q * k * 8);
    p.off_po = ws.take((size_t)p.nblk * Q * k * 8);
    p.total = ws.off;
    return p;
}

int scope_check(vm_memory *m, const void *queries, int Q, int k, const int64_t *scope_lo, const int64_t *scope_hi,
                int score_mode, const double *out_scores, const int64_t *out_rows, const void *workspace,
                size_t workspace_bytes, const char *who) {
    return vm_topk_check(m, m->tag ? nullptr : "tagged (vm_memory_create_tagged)",
                         queries && scope_lo && scope_hi && out_scores && out_rows && Q > 0, queries, k, SKMAX,
                         VM_ERR_INVALID, score_mode, workspace, workspace_bytes, scope_plan(m, Q, k).total, who);
}

int scope_redo(vm_memory *m, const SPlan &p, const void *queries, int Q, int k, const int64_t *scope_lo,
               const int64_t *scope_hi, int use_min, double min_score, int score_mode, int64_t row_stride,
               int64_t row_offset, double *out_scores, int64_t *out_rows, char *ws, hipStream_t st) {
    vm_ctx *ctx = m->ctx;
    vm_prof_scope prof(ctx, VM_PROF_TOPK_EXACT, st);
    const int32_t *flags = (const int32_t *)(ws + p.off_flags);
    double *part_s = (double *)(ws + p.off_ps);
    int64_t *part_o = (int64_t *)(ws + p.off_po);
    if (int rc = vm_topk_redo_scan(m, queries, Q, k, scope_lo, scope_hi, flags, p.nblk, part_s, part_o, st)) return rc;
    return vm_topk_redo_merge(m, part_s, part_o, p.nblk, Q, k, flags, use_min, min_score, score_mode, row_stride,
                              row_offset, out_scores, out_rows, nullptr, nullptr, st);
}

template <int DT>
int scope_topk(vm_memory *m, const void *queries, int Q, int k, const int64_t *scope_lo, const int64_t *scope_hi,
               int use_min, double min_score, int score_mode, int64_t row_stride, int64_t row_offset,
               double *out_scores, int64_t *out_rows, int32_t *out_uncertified, int32_t *out_query_flags, char *ws,
               hipStream_t st) {
    vm_ctx *ctx = m->ctx;
    const SPlan p = scope_plan(m, Q, k);
    uint32_t *F = (uint32_t *)ws;
    int *cand_o = (int *)(ws + p.off_co);
    uint32_t *cand_k = (uint32_t *)(ws + p.off_ck);
    int *cand_n = (int *)(ws + p.off_cn);
    int *flags = (int *)(ws + p.off_flags);
    {
        vm_prof_scope prof(ctx, VM_PROF_TOPK_SCAN, st);
        const int rc = vm_tile_scan<DT, ScopeScan>(m, p, queries, Q, {m->tag, scope_lo, scope_hi, p.fstride, F}, st);
        if (rc != VM_OK) return rc;
    }
    {
        vm_prof_scope prof(ctx, VM_PROF_TOPK_FINALIZE, st);
        uint32_t *cut = (uint32_t *)(ws + p.off_cut);
        int *ccount = (int *)(ws + p.off_cc);
        unsigned long long *cbuf = (unsigned long long *)(ws + p.off_cbuf);
        scope_cut_kernel<<<Q, SEL_THREADS, 0, st>>>(m->d_total, m->cap, m->ring, F, p.fstride, p.M + 1, cut, ccount);
        VM_LAUNCH_CHECK(ctx);
        scope_compact_kernel<<<dim3(p.cmp_slices, Q), CMP_THREADS, 0, st>>>(m->d_total, m->cap, m->ring, F, p.fstride,
                                                                            cut, ccount, cbuf);
        VM_LAUNCH_CHECK(ctx);
        scope_select_kernel<<<Q, SEL_THREADS, 0, st>>>(p.M + 1, ccount, cbuf, cand_o, cand_k, cand_n);
        VM_LAUNCH_CHECK(ctx);
        scope_finalize_kernel<DT><<<Q, SF_THREADS, (size_t)m->D * 2, st>>>(
            m->rows, m->norm64, (const uint16_t *)queries, m->d_total, m->cap, m->ring, m->D, cand_o, cand_k, cand_n,
            p.M, k, use_min, min_score, score_mode, row_stride, row_offset, out_scores, out_rows, out_uncertified, flags,
            out_query_flags);
        VM_LAUNCH_CHECK(ctx);
    }
    return scope_redo(m, p, queries, Q, k, scope_lo, scope_hi, use_min, min_score, score_mode, row_stride,
                          row_offset, out_scores, out_rows, ws, st);
}

}  // namespace

extern "C" size_t vm_topk_scoped_workspace_bytes(const vm_memory *m, int Q, int k) {
    if (!m || Q <= 0 || k <= 0 || k > SKMAX) return 0;
    return scope_plan(m, Q, k).total;
}

extern "C" int vm_topk_cosine_scoped(vm_memory *m, const void *queries, int Q, int k, const int64_t *scope_lo,
                                     const int64_t *scope_hi, int use_min_score, double min_score, int score_mode,
                                     int64_t row_stride, int64_t row_offset, double *out_scores, int64_t *out_rows,
                                     int32_t *out_uncertified, int32_t *out_query_flags, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    if (!m) return VM_ERR_INVALID;
    int rc = scope_check(m, queries, Q, k, scope_lo, scope_hi, score_mode, out_scores, out_rows, workspace,
                         workspace_bytes, "vm_topk_cosine_scoped");
    if (rc != VM_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    return vm_by_dtype(m, [&](auto dt) {
        return scope_topk<decltype(dt)::value>(m, queries, Q, k, scope_lo, scope_hi, use_min_score, min_score,
                                               score_mode, row_stride, row_offset, out_scores, out_rows,
                                               out_uncertified, out_query_flags, (char *)workspace, st);
    });
}

extern "C" int vm_topk_cosine_scoped_exact(vm_memory *m, const void *queries, int Q, int k, const int64_t *scope_lo,
                                           const int64_t *scope_hi, int use_min_score, double min_score, int score_mode,
                                           int64_t row_stride, int64_t row_offset, double *out_scores,
                                           int64_t *out_rows, void *workspace, size_t workspace_bytes, void *stream) {
    if (!m) return VM_ERR_INVALID;
    int rc = scope_check(m, queries, Q, k, scope_lo, scope_hi, score_mode, out_scores, out_rows, workspace,
                         workspace_bytes, "vm_topk_cosine_scoped_exact");
    if (rc != VM_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    vm_ctx *ctx = m->ctx;
    const SPlan p = scope_plan(m, Q, k);
    char *ws = (char *)workspace;
    scope_fill_flags_kernel<<<(Q + 255) / 256, 256, 0, st>>>((int32_t *)(ws + p.off_flags), Q);
    VM_LAUNCH_CHECK(ctx);
    return scope_redo(m, p, queries, Q, k, scope_lo, scope_hi, use_min_score, min_score, score_mode, row_stride,
                      row_offset, out_scores, out_rows, ws, st);
}
