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
#include "topk_scope_select.h"  // the select stage (cut, compaction, selection) and the finalize: shared
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

// ---- redo --------------------------------------------------------------------------------------------------
__global__ void scope_fill_flags_kernel(int32_t *__restrict__ flags, int Q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Q) flags[i] = 1;
}

// ---- host --------------------------------------------------------------------------------------------------
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
