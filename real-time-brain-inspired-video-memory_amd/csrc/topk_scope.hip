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
#include "topk_scope_select.h"  // the select stage (cut, compaction, selection) and the finalize: topk_key_image.hip
#include "topk_tile_scan.h"

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
    using QState = TagQState<QT>;
    struct View {};
    template <class QS>
    static __device__ __forceinline__ void load_query(QS &qs, const Args &a, int i, int q, bool live) {
        load_tag_scope(qs, a.scope_lo, a.scope_hi, i, q, live);
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

// ---- host --------------------------------------------------------------------------------------------------
int scope_check(vm_memory *m, const RowCall &c, const int64_t *scope_lo, const int64_t *scope_hi, size_t workspace_bytes,
                const char *who) {
    return vm_topk_check(m, m->tag ? nullptr : "tagged (vm_memory_create_tagged)",
                         c.queries && scope_lo && scope_hi && c.out_scores && c.out_rows && c.Q > 0, c.queries, c.k,
                         SKMAX, VM_ERR_INVALID, c.score_mode, c.ws, workspace_bytes, vm_key_image_plan(m, c.Q, c.k).total, who);
}

// both entry points: the fast form (topk_scope_select.h key_image_topk under ScopeScan) or the exhaustive one
int scope_entry(vm_memory *m, const RowCall &c, const int64_t *scope_lo, const int64_t *scope_hi, size_t workspace_bytes,
                bool exact, const char *who) {
    if (!m) return VM_ERR_INVALID;
    if (int rc = scope_check(m, c, scope_lo, scope_hi, workspace_bytes, who)) return rc;
    const TagScope sc = {m->tag, scope_lo, scope_hi};
    if (exact) return key_image_exact(m, c, sc);
    return vm_by_dtype(m, [&](auto dt) {
        return key_image_topk<decltype(dt)::value, ScopeScan>(m, c, {m->tag, scope_lo, scope_hi, 0, nullptr}, sc);
    });
}

}  // namespace

extern "C" size_t vm_topk_scoped_workspace_bytes(const vm_memory *m, int Q, int k) {
    if (!m || Q <= 0 || k <= 0 || k > SKMAX) return 0;
    return vm_key_image_plan(m, Q, k).total;
}

extern "C" int vm_topk_cosine_scoped(vm_memory *m, const void *queries, int Q, int k, const int64_t *scope_lo,
                                     const int64_t *scope_hi, int use_min_score, double min_score, int score_mode,
                                     int64_t row_stride, int64_t row_offset, double *out_scores, int64_t *out_rows,
                                     int32_t *out_uncertified, int32_t *out_query_flags, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    const RowCall c = {queries,    Q,          k,          use_min_score, min_score,       score_mode,
                       row_stride, row_offset, out_scores, out_rows,      out_uncertified, out_query_flags,
                       (char *)workspace, (hipStream_t)stream};
    return scope_entry(m, c, scope_lo, scope_hi, workspace_bytes, false, "vm_topk_cosine_scoped");
}

extern "C" int vm_topk_cosine_scoped_exact(vm_memory *m, const void *queries, int Q, int k, const int64_t *scope_lo,
                                           const int64_t *scope_hi, int use_min_score, double min_score, int score_mode,
                                           int64_t row_stride, int64_t row_offset, double *out_scores,
                                           int64_t *out_rows, void *workspace, size_t workspace_bytes, void *stream) {
    const RowCall c = {queries,    Q,          k,          use_min_score, min_score, score_mode,
                       row_stride, row_offset, out_scores, out_rows,      nullptr,   nullptr,
                       (char *)workspace, (hipStream_t)stream};
    return scope_entry(m, c, scope_lo, scope_hi, workspace_bytes, true, "vm_topk_cosine_scoped_exact");
}
