// Span cosine top-k: the k best rows among those whose ROW ID lies in the query's inclusive span [row_lo, row_hi]
// (include/vidmem.h vm_topk_cosine_span).  Row ids are append order and append order is time, so a span is "the past
// before this frame": what a stored frame resembles in its own past, other than a moment ago.
//
// The scoped search with a third predicate (vm_internal.h RowSpan), built from the same parts as topk_scope.hip and
// topk_mask.hip:
//   scan     : topk_tile_scan.h under the SpanScan policy below.  Whether a 16-row tile holds a wanted row follows from
//              arithmetic on the tile's slots and the ring's head: the pre-test reads NO global memory (against 128 bytes
//              of tags in the scoped search, 2 bytes of mask per query in the masked one).  A tile no query wants is
//              skipped without reading its rows and only zeroes its keys.  Otherwise fp32 MFMA scores,
//              F[q][slot] = okey32(score) for a live row in the query's span, 0 for any other
//   select   : topk_key_image.hip, through topk_scope_select.h
//   finalize : topk_key_image.hip's scope_finalize_kernel.  Certified when the span holds at most M live rows,
//              or when the exact k-th score clears the (M+1)-th IN-SPAN fp32 score / ||q|| by cert_eps(D), strictly.  Rows
//              outside the span have key 0 and never reach the certificate
//   redo     : vm_topk_redo_scan under the RowSpan predicate (topk_exact.hip), then vm_topk_redo_merge
// A span is clamped to the live rows where it is read: ids below the oldest row, at or past the row count, or negative
// are ignored.  Every launch reads the row count and the spans from the device and sizes its grid from the capacity:
// capturable.
#include "topk_scope_select.h"
#include "topk_tile_scan.h"

namespace {

// ---- scan --------------------------------------------------------------------------------------------------
// The span policy of the tile scan: four keys per lane, F[q * fstride + slot] = the order-preserving key of the fp32
// score, or 0 when the row's age order is outside the query's bounds or the slot is past the live rows.  The per-query
// state is the span as bounds on the AGE ORDER (order_span), in 32 bits: an order is below the capacity, which the select
// stage's composites hold in an int already.  The empty span is INT_MAX .. INT_MIN, so that it overlaps no run of orders.
struct SpanScan {
    struct Args {
        const int64_t *row_lo, *row_hi, *d_total;
        int64_t cap;
        int ring;
        int64_t fstride;
        uint32_t *F;
    };
    template <int QT>
    struct QState {
        alignas(16) int lo[QT * 16], hi[QT * 16];
        int head;  // the RingView's, for the slot -> order arithmetic of skip_tile and the epilogue
    };
    struct View {};
    template <class QS>
    static __device__ __forceinline__ void load_query(QS &qs, const Args &a, int i, int q, bool live) {
        const RowSpan::Q s = RowSpan{a.row_lo, a.row_hi, a.d_total, a.cap, a.ring}.at(live ? q : 0);
        const bool some = live && s.lo <= s.hi;
        qs.lo[i] = some ? (int)s.lo : INT_MAX;
        qs.hi[i] = some ? (int)s.hi : INT_MIN;
        if (i == 0) qs.head = (int)s.rv.head;
    }
    static __device__ __forceinline__ View view(const Args &, const RingView &) { return {}; }
    // age order of the live row in slot p (order_of in 32 bits; head > 0 only in a wrapped ring)
    static __device__ __forceinline__ int order(int p, int head, int cap) { return p - head + (p < head ? cap : 0); }
    // the age orders of the lane's four slots p0 .. p0 + 3; -1, below every bound, for a slot past the live rows
    static __device__ __forceinline__ void lane_orders(int (&oj)[4], int p0, int n, int head, int cap) {
#pragma unroll
        for (int j = 0; j < 4; ++j) oj[j] = p0 + j < n ? order(p0 + j, head, cap) : -1;
    }
    template <int QT>
    static __device__ __forceinline__ bool skip_tile(const QState<QT> &qs, const Args &a, const TileLane &l) {
        // the tile and the head are the same in every lane: scalar, so that nothing of them stays in VGPRs across the
        // MFMA loop
        const int t0 = __builtin_amdgcn_readfirstlane((int)l.tile) * 16;
        const int head = __builtin_amdgcn_readfirstlane(qs.head);
        const int n = (int)l.n;
        const int t1 = t0 + 15 < n - 1 ? t0 + 15 : n - 1;  // the tile's last live slot; >= t0
        bool hit = false;
        // both tests read the bounds in the epilogue's lane layout - lane (r16, h) has query 16 t + r16 - so that one LDS
        // address serves all three
        if (head > t0 && head <= t1) {
            // the ring's head seam inside the tile: two runs of orders.  Per row, as tile_in_scope does with tags, with the
            // row's order in place of its tag: the lane tests its slots 4h .. 4h+3 of the tile
            int oj[4];
            lane_orders(oj, t0 + 4 * l.h, n, head, (int)a.cap);
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                const int lo = qs.lo[16 * t + l.r16], hi = qs.hi[16 * t + l.r16];
#pragma unroll
                for (int j = 0; j < 4; ++j) hit |= lo <= oj[j] && oj[j] <= hi;
            }
        } else {
            // one run of orders o0 .. o0 + (t1 - t0), against the bounds of every block query
            const int o0 = order(t0, head, (int)a.cap);
#pragma unroll
            for (int t = 0; t < QT; ++t) hit |= qs.lo[16 * t + l.r16] <= o0 + (t1 - t0) && o0 <= qs.hi[16 * t + l.r16];
        }
        if (__ballot(hit) != 0ull) return false;
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
        const int head = __builtin_amdgcn_readfirstlane(qs.head);
        int oj[4];
        lane_orders(oj, (int)l.p0(), (int)l.n, head, (int)a.cap);
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const int q = l.q0 + 16 * t + l.r16;
            if (q >= l.Q) continue;
            const int lo = qs.lo[16 * t + l.r16], hi = qs.hi[16 * t + l.r16];
            uint32_t key[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) key[j] = (lo <= oj[j] && oj[j] <= hi) ? okey32(s[t][j]) : 0u;
            *reinterpret_cast<uint4 *>(a.F + (size_t)q * a.fstride + l.p0()) = make_uint4(key[0], key[1], key[2], key[3]);
        }
    }
};

// ---- host --------------------------------------------------------------------------------------------------
int span_check(vm_memory *m, const RowCall &c, const int64_t *row_lo, const int64_t *row_hi, size_t workspace_bytes,
               const char *who) {
    return vm_topk_check(m, nullptr, c.queries && row_lo && row_hi && c.out_scores && c.out_rows && c.Q > 0, c.queries,
                         c.k, SKMAX, VM_ERR_INVALID, c.score_mode, c.ws, workspace_bytes, vm_key_image_plan(m, c.Q, c.k).total,
                         who);
}

// both entry points: the fast form (topk_scope_select.h key_image_topk under SpanScan; the scoped search's workspace, the
// same stages over the same key image) or the exhaustive one
int span_entry(vm_memory *m, const RowCall &c, const int64_t *row_lo, const int64_t *row_hi, size_t workspace_bytes,
               bool exact, const char *who) {
    if (!m) return VM_ERR_INVALID;
    if (int rc = span_check(m, c, row_lo, row_hi, workspace_bytes, who)) return rc;
    const RowSpan sp = {row_lo, row_hi, m->d_total, m->cap, m->ring};
    if (exact) return key_image_exact(m, c, sp);
    return vm_by_dtype(m, [&](auto dt) {
        return key_image_topk<decltype(dt)::value, SpanScan>(m, c, {row_lo, row_hi, m->d_total, m->cap, m->ring, 0, nullptr},
                                                             sp);
    });
}

}  // namespace

extern "C" size_t vm_topk_span_workspace_bytes(const vm_memory *m, int Q, int k) {
    if (!m || Q <= 0 || k <= 0 || k > SKMAX) return 0;
    return vm_key_image_plan(m, Q, k).total;
}

extern "C" int vm_topk_cosine_span(vm_memory *m, const void *queries, int Q, int k, const int64_t *row_lo,
                                   const int64_t *row_hi, int use_min_score, double min_score, int score_mode,
                                   int64_t row_stride, int64_t row_offset, double *out_scores, int64_t *out_rows,
                                   int32_t *out_uncertified, int32_t *out_query_flags, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    const RowCall c = {queries,    Q,          k,          use_min_score, min_score,       score_mode,
                       row_stride, row_offset, out_scores, out_rows,      out_uncertified, out_query_flags,
                       (char *)workspace, (hipStream_t)stream};
    return span_entry(m, c, row_lo, row_hi, workspace_bytes, false, "vm_topk_cosine_span");
}

extern "C" int vm_topk_cosine_span_exact(vm_memory *m, const void *queries, int Q, int k, const int64_t *row_lo,
                                         const int64_t *row_hi, int use_min_score, double min_score, int score_mode,
                                         int64_t row_stride, int64_t row_offset, double *out_scores, int64_t *out_rows,
                                         void *workspace, size_t workspace_bytes, void *stream) {
    const RowCall c = {queries,    Q,          k,          use_min_score, min_score, score_mode,
                       row_stride, row_offset, out_scores, out_rows,      nullptr,   nullptr,
                       (char *)workspace, (hipStream_t)stream};
    return span_entry(m, c, row_lo, row_hi, workspace_bytes, true, "vm_topk_cosine_span_exact");
}
