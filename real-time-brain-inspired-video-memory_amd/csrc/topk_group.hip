// Grouped cosine top-k: the k best GROUPS (video chunks) of a grouped memory, one hit per group (include/vidmem.h).
//
// The row ranking is vm_topk_cosine's (src/components/pre_llm_injector.py:346-388, retriever_hybrid.py:293-306); a
// group's score is the exact max over its rows and its representative the lowest row id reaching that max.  Same
// two-stage, certified design as topk.hip; the key images, the block-wide selection, the plan
// scaffold and the argument check are topk_select.h's, shared with topk_scope.hip; the scan is topk_tile_scan.h's, shared
// with topk_scope.hip and range.hip (GroupScan below is its policy); the run folding, the radix select, the finalize, the
// redo scan and the plan live in topk_group_parts.h, the table and the compaction in topk_group_parts.hip, all shared with
// topk_group_scope.hip:
//   table    : first age order of every live group (groups are runs of equal ordinals, memory.hip) + clears the maxima
//   scan     : fp32 MFMA scores with the list scan's numerics (the same instruction over the same operand layout, then
//              x 1/||row||), folded into per-(query, group) fp32 maxima with one atomic max per run of a 16-row tile
//   select   : per query, the best M + 1 groups by (fp32 max desc, group asc): a cut from a sample of the maxima, a
//              parallel compaction of every group at or above it, a block-wide selection (radix over all maxima if too many)
//   finalize : every row of the best M groups re-scored exactly in fp64 (one rounding per product and per partial sum,
//              left to right; norm64), exact group max + representative, ordered, k kept.  Certified when the exact
//              k-th group score clears the (M+1)-th group's fp32 max / ||q|| by topk.hip's bound 2 (D + 8) 2^-24
//   redo     : flagged queries (gap or candidate-row overflow) scored exhaustively, group-aligned row slices per
//              block, segmented max in LDS, stable top-k per slice, then the one merge of every redo
//              (vm_topk_redo_merge, topk_exact.hip).  Reads flags and counts on the device.
// Every launch reads the row count from the device and sizes its grid from the capacity: capturable.
#include "topk_group_parts.h"

namespace {

// ---- scan --------------------------------------------------------------------------------------------------
// The grouped policy of the tile scan (topk_tile_scan.h).  Instead of a key per row, each lane folds its 4 consecutive
// rows into runs of one group and raises F[q * ng + group] with one atomic max per run.
struct GroupScan {
    struct Args {
        const int64_t *gord;
        uint32_t *F;
    };
    template <int QT>
    struct QState {};
    using View = GroupView;
    template <class QS>
    static __device__ __forceinline__ void load_query(QS &, const Args &, int, int, bool) {}
    static __device__ __forceinline__ View view(const Args &a, const RingView &rv) { return group_view(rv, a.gord); }
    template <int QT>
    static __device__ __forceinline__ bool skip_tile(const QState<QT> &, const Args &, const TileLane &) {
        return false;
    }
    template <int QT>
    static __device__ __forceinline__ void epilogue(const QState<QT> &, const Args &a, const View &gv,
                                                    const TileLane &l, const float (&s)[QT][4]) {
        group_fold_runs<QT>(a.gord, a.F, gv, l, s, [](int, int, float sc) { return okey32(sc); });
    }
};

// ---- select ------------------------------------------------------------------------------------------------
// Per query, the best take = min(M + 1, ng) groups by (fp32 max desc, group asc), as 64-bit composites
// key << 32 | ~group (topk_select.h).  cut: the take-th best composite of a strided sample of SEL_SAMPLE groups (all of
// them when there are fewer) - at least take groups reach it; compact: every group at or above the cut, from many
// blocks; final: the take-th largest key among those (ties by group), the take best kept (select_best).  A query with
// more than SEL_CAP groups at its cut runs the exact radix select below over all its groups instead (slow, any input).

// One block per query: cut = key T << 32, T = the take-th largest fp32-max key of a strided sample of SEL_SAMPLE groups
// (all of them when there are fewer).  At least take groups have a key >= T (ties at T included, whatever their group).
__global__ void __launch_bounds__(SEL_THREADS)
    group_cut_kernel(const int64_t *__restrict__ d_total, int64_t cap, int ring, const int64_t *__restrict__ gord,
                     const uint32_t *__restrict__ F, int M1, unsigned long long *__restrict__ cut,
                     int *__restrict__ ccount) {
    constexpr int PER = SEL_SAMPLE / SEL_THREADS;
    const int q = blockIdx.x, lane = threadIdx.x;
    const GroupView gv = group_view(d_total, cap, ring, gord);
    const int64_t ng = gv.ng;
    const uint32_t *Fq = F + (size_t)q * ng;
    const int cnt = (int)(ng < SEL_SAMPLE ? ng : SEL_SAMPLE);
    uint32_t v[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = j * SEL_THREADS + lane;
        v[j] = i < cnt ? Fq[ng <= SEL_SAMPLE ? i : (int64_t)i * ng / SEL_SAMPLE] : 0u;
    }
    const int take = cnt < M1 ? cnt : M1;
    const uint32_t T = take > 0 ? block_kth_u32<SEL_THREADS>(v, take) : 0xffffffffu;
    if (lane == 0) {
        cut[q] = (unsigned long long)T << 32;
        ccount[q] = 0;
    }
}

// One block per query: the best take groups of the compacted list, or of all groups when the list overflowed.
__global__ void __launch_bounds__(SEL_THREADS)
    group_select_final_kernel(const int64_t *__restrict__ d_total, int64_t cap, int ring,
                              const int64_t *__restrict__ gord, const uint32_t *__restrict__ F, int M1,
                              const int *__restrict__ ccount, const unsigned long long *__restrict__ cbuf,
                              int *__restrict__ cand_g, uint32_t *__restrict__ cand_k, int *__restrict__ cand_n) {
    const int q = blockIdx.x, tid = threadIdx.x;
    const GroupView gv = group_view(d_total, cap, ring, gord);
    const int ng = (int)gv.ng;
    int *og = cand_g + (size_t)q * GCMAX;
    uint32_t *ok = cand_k + (size_t)q * GCMAX;
    const int take = ng < M1 ? ng : M1;
    if (tid == 0) cand_n[q] = take;
    const int cnt = ccount[q];
    if (cnt > SEL_CAP) {
        radix_select_all(F + (size_t)q * ng, ng, take, og, ok);
        return;
    }
    select_best<SEL_THREADS, SEL_CAP, GCMAX>(cbuf + (size_t)q * SEL_CAP, cnt, take, og, ok);
}

// ---- host --------------------------------------------------------------------------------------------------
int group_check(vm_memory *m, const GroupCall &c, size_t workspace_bytes, const char *who) {
    return vm_topk_check(m, m->gkey ? nullptr : "grouped (vm_memory_create_grouped)",
                         c.queries && c.out_scores && c.out_rows && c.Q > 0 && c.k > 0, c.queries, c.k, GKMAX,
                         VM_ERR_UNSUPPORTED, c.score_mode, c.ws, workspace_bytes, group_plan(m, c.Q, c.k).total, who);
}

// both entry points: the fast form (topk_group_parts.h grouped_topk under GroupScan) or the exhaustive one
int group_entry(vm_memory *m, const GroupCall &c, size_t workspace_bytes, bool exact, const char *who) {
    if (!m) return VM_ERR_INVALID;
    if (int rc = group_check(m, c, workspace_bytes, who)) return rc;
    if (exact) return grouped_exact(m, c, NoScope{});
    return vm_by_dtype(m, [&](auto dt) {
        return grouped_topk<decltype(dt)::value, GroupScan, group_cut_kernel, group_select_final_kernel>(
            m, c, {m->gord, nullptr}, NoScope{});
    });
}

}  // namespace

extern "C" size_t vm_topk_grouped_workspace_bytes(const vm_memory *m, int Q, int k) {
    if (!m || Q <= 0 || k <= 0 || k > GKMAX) return 0;
    return group_plan(m, Q, k).total;
}

extern "C" int vm_topk_cosine_grouped(vm_memory *m, const void *queries, int Q, int k, int use_min_score,
                                      double min_score, int score_mode, double *out_scores, int64_t *out_rows,
                                      int64_t *out_keys, int32_t *out_uncertified, int32_t *out_query_flags,
                                      void *workspace, size_t workspace_bytes, void *stream) {
    const GroupCall c = {queries,  Q,        k,         use_min_score,   min_score,       score_mode, out_scores,
                         out_rows, out_keys, out_uncertified, out_query_flags, (char *)workspace, (hipStream_t)stream};
    return group_entry(m, c, workspace_bytes, false, "vm_topk_cosine_grouped");
}

extern "C" int vm_topk_cosine_grouped_exact(vm_memory *m, const void *queries, int Q, int k, int use_min_score,
                                            double min_score, int score_mode, double *out_scores, int64_t *out_rows,
                                            int64_t *out_keys, void *workspace, size_t workspace_bytes, void *stream) {
    const GroupCall c = {queries,  Q,        k,       use_min_score, min_score,         score_mode, out_scores,
                         out_rows, out_keys, nullptr, nullptr,       (char *)workspace, (hipStream_t)stream};
    return group_entry(m, c, workspace_bytes, true, "vm_topk_cosine_grouped_exact");
}
