// Scoped grouped cosine top-k: the k best GROUPS of a tagged, grouped memory among the rows whose TAG lies in the
// query's inclusive range [lo, hi], one hit per group (include/vidmem.h) - "the k best scenes of video 7 between minute
// 10 and minute 20".
//
// The row ranking is vm_topk_cosine_scoped's (in-scope live rows only); a group's score is the exact max over its
// IN-SCOPE rows and its representative the lowest in-scope row id reaching that max.  Groups are what they are everywhere
// else - runs of equal ordinals over ALL live rows (memory.hip): a scope hides rows, it neither splits nor merges groups,
// and a group with no in-scope row does not exist for the query.  The five stages of topk_group.hip
// with the tag predicate of topk_scope.hip; shared with the first through topk_group_parts.h (table, run folding,
// compaction, radix select, finalize, redo scan, plan), with both through topk_select.h and topk_tile_scan.h:
//   table    : topk_group.hip's - first age order of every live group; clears the per-(query, group) maxima to 0, and 0
//              stays "no in-scope row seen" (every real score's key is above 0, topk_select.h okey32)
//   scan     : GroupScopeScan below, the fourth policy of the tile scan.  Per 16-row tile the wave first tests the tile's
//              16 tags against the scopes of its query tile: a tile with no (row, query) pair in scope is skipped without
//              reading its rows and writes nothing.  Otherwise the grouped run folding with the key of an out-of-scope
//              (query, row) pair replaced by 0: the mask is per (query, row), the run structure per row, and an atomic
//              max with 0 is a no-op, so the runs need no special case
//   select   : only groups with a non-zero key are candidates.  The cut is at least key 1 (gscope_cut_kernel), so the
//              compaction never takes an empty group; the candidate count is min(M + 1, groups at or above the cut)
//   finalize : the in-scope rows of the best M candidate groups re-scored exactly; exact max and lowest row over those
//              rows only; certified against the (M+1)-th candidate's fp32 max over ITS in-scope rows, outright when
//              there is no (M+1)-th in-scope group.  GROWCAP counts ALL rows of the candidate groups, in scope or not:
//              the rows to visit are found from the groups' lengths before any tag is read
//   redo     : the grouped redo scan with the tag predicate: a group, or the carried part of one, with no in-scope row
//              yields no entry.  Then vm_topk_redo_merge with keys.
// Every launch reads the row count and the scopes from the device and sizes its grid from the capacity: capturable.
#include "topk_group_parts.h"

namespace {

// ---- scan --------------------------------------------------------------------------------------------------
struct GroupScopeScan {
    struct Args {
        const int64_t *gord, *tag, *scope_lo, *scope_hi;
        uint32_t *F;
    };
    template <int QT>
    using QState = TagQState<QT>;
    using View = GroupView;
    template <class QS>
    static __device__ __forceinline__ void load_query(QS &qs, const Args &a, int i, int q, bool live) {
        load_tag_scope(qs, a.scope_lo, a.scope_hi, i, q, live);
    }
    static __device__ __forceinline__ View view(const Args &a, const RingView &rv) { return group_view(rv, a.gord); }
    template <int QT>
    static __device__ __forceinline__ bool skip_tile(const QState<QT> &qs, const Args &a, const TileLane &l) {
        return !tile_in_scope<QT>(a.tag, qs.lo, qs.hi, l);  // the table kernel cleared the maxima: nothing to write
    }
    template <int QT>
    static __device__ __forceinline__ void epilogue(const QState<QT> &qs, const Args &a, const View &gv,
                                                    const TileLane &l, const float (&s)[QT][4]) {
        int64_t tj[4];  // p0 + 3 is below the columns' padding; a row past the live ones is masked by the run folding
#pragma unroll
        for (int j = 0; j < 4; ++j) tj[j] = a.tag[l.p0() + j];
        group_fold_runs<QT>(a.gord, a.F, gv, l, s, [&](int t, int j, float sc) {
            return in_scope(tj[j], qs.lo[16 * t + l.r16], qs.hi[16 * t + l.r16]) ? okey32(sc) : 0u;
        });
    }
};

// ---- select ------------------------------------------------------------------------------------------------
// One block per query: group_cut_kernel (topk_group.hip) with the cut held at key 1 or above.  T = the (M+1)-th largest
// fp32-max key of a strided sample of SEL_SAMPLE groups (all of them when there are fewer); under a narrow scope most
// sampled maxima are 0, and a cut of 0 would send every empty group to the compaction and every query to the radix path.
// With T >= 1 at least min(M + 1, groups with an in-scope row) groups have a key >= T, and no empty group has.
__global__ void __launch_bounds__(SEL_THREADS)
    gscope_cut_kernel(const int64_t *__restrict__ d_total, int64_t cap, int ring, const int64_t *__restrict__ gord,
                      const uint32_t *__restrict__ F, int M1, unsigned long long *__restrict__ cut,
                      int *__restrict__ ccount) {
    constexpr int PER = SEL_SAMPLE / SEL_THREADS;
    const int q = blockIdx.x, tid = threadIdx.x;
    const GroupView gv = group_view(d_total, cap, ring, gord);
    const int64_t ng = gv.ng;
    const uint32_t *Fq = F + (size_t)q * ng;
    const int cnt = (int)(ng < SEL_SAMPLE ? ng : SEL_SAMPLE);
    uint32_t v[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = j * SEL_THREADS + tid;
        v[j] = i < cnt ? Fq[ng <= SEL_SAMPLE ? i : (int64_t)i * ng / SEL_SAMPLE] : 0u;
    }
    const uint32_t T = block_kth_u32<SEL_THREADS>(v, M1);  // 0 when the sample holds fewer than M1 non-empty groups
    if (tid == 0) {
        cut[q] = (unsigned long long)(T ? T : 1u) << 32;
        ccount[q] = 0;
    }
}

// One block per query: the best take = min(M + 1, groups at or above the cut) groups of the compacted list.  When the
// list overflowed, the radix select of the best M + 1 over all groups instead.  The cut is at least key 1, so an
// overflow means more than CMP_LCAP non-empty groups (one compaction block's hits, or SEL_CAP of them together) - more
// than M + 1 <= GCMAX: the M + 1 best keys are all non-zero and no empty group is taken.
__global__ void __launch_bounds__(SEL_THREADS)
    gscope_select_final_kernel(const int64_t *__restrict__ d_total, int64_t cap, int ring,
                               const int64_t *__restrict__ gord, const uint32_t *__restrict__ F, int M1,
                               const int *__restrict__ ccount, const unsigned long long *__restrict__ cbuf,
                               int *__restrict__ cand_g, uint32_t *__restrict__ cand_k, int *__restrict__ cand_n) {
    const int q = blockIdx.x, tid = threadIdx.x;
    const GroupView gv = group_view(d_total, cap, ring, gord);
    const int ng = (int)gv.ng;
    int *og = cand_g + (size_t)q * GCMAX;
    uint32_t *ok = cand_k + (size_t)q * GCMAX;
    const int cnt = ccount[q];
    if (cnt > SEL_CAP) {  // uniform
        if (tid == 0) cand_n[q] = M1;
        radix_select_all(F + (size_t)q * ng, ng, M1, og, ok);
        return;
    }
    const int take = cnt < M1 ? cnt : M1;
    if (tid == 0) cand_n[q] = take;
    select_best<SEL_THREADS, SEL_CAP, GCMAX>(cbuf + (size_t)q * SEL_CAP, cnt, take, og, ok);
}

// ---- host --------------------------------------------------------------------------------------------------
int gscope_check(vm_memory *m, const GroupCall &c, const int64_t *scope_lo, const int64_t *scope_hi,
                 size_t workspace_bytes, const char *who) {
    const char *missing = !m->tag    ? "tagged (vm_memory_create_tagged)"
                          : !m->gkey ? "grouped (vm_memory_create_tagged with grouped != 0)"
                                     : nullptr;
    return vm_topk_check(m, missing, c.queries && scope_lo && scope_hi && c.out_scores && c.out_rows && c.Q > 0,
                         c.queries, c.k, GKMAX, VM_ERR_INVALID, c.score_mode, c.ws, workspace_bytes,
                         group_plan(m, c.Q, c.k).total, who);
}

// both entry points: the fast form (topk_group_parts.h grouped_topk under GroupScopeScan) or the exhaustive one
int gscope_entry(vm_memory *m, const GroupCall &c, const int64_t *scope_lo, const int64_t *scope_hi,
                 size_t workspace_bytes, bool exact, const char *who) {
    if (!m) return VM_ERR_INVALID;
    if (int rc = gscope_check(m, c, scope_lo, scope_hi, workspace_bytes, who)) return rc;
    const TagScope sc = {m->tag, scope_lo, scope_hi};
    if (exact) return grouped_exact(m, c, sc);
    return vm_by_dtype(m, [&](auto dt) {
        return grouped_topk<decltype(dt)::value, GroupScopeScan, gscope_cut_kernel, gscope_select_final_kernel>(
            m, c, {m->gord, m->tag, scope_lo, scope_hi, nullptr}, sc);
    });
}

}  // namespace

extern "C" size_t vm_topk_grouped_scoped_workspace_bytes(const vm_memory *m, int Q, int k) {
    if (!m || Q <= 0 || k <= 0 || k > GKMAX) return 0;
    return group_plan(m, Q, k).total;
}

extern "C" int vm_topk_cosine_grouped_scoped(vm_memory *m, const void *queries, int Q, int k, const int64_t *scope_lo,
                                             const int64_t *scope_hi, int use_min_score, double min_score,
                                             int score_mode, double *out_scores, int64_t *out_rows, int64_t *out_keys,
                                             int32_t *out_uncertified, int32_t *out_query_flags, void *workspace,
                                             size_t workspace_bytes, void *stream) {
    const GroupCall c = {queries,  Q,        k,         use_min_score,   min_score,       score_mode, out_scores,
                         out_rows, out_keys, out_uncertified, out_query_flags, (char *)workspace, (hipStream_t)stream};
    return gscope_entry(m, c, scope_lo, scope_hi, workspace_bytes, false, "vm_topk_cosine_grouped_scoped");
}

extern "C" int vm_topk_cosine_grouped_scoped_exact(vm_memory *m, const void *queries, int Q, int k,
                                                   const int64_t *scope_lo, const int64_t *scope_hi, int use_min_score,
                                                   double min_score, int score_mode, double *out_scores,
                                                   int64_t *out_rows, int64_t *out_keys, void *workspace,
                                                   size_t workspace_bytes, void *stream) {
    const GroupCall c = {queries,  Q,        k,       use_min_score, min_score,         score_mode, out_scores,
                         out_rows, out_keys, nullptr, nullptr,       (char *)workspace, (hipStream_t)stream};
    return gscope_entry(m, c, scope_lo, scope_hi, workspace_bytes, true, "vm_topk_cosine_grouped_scoped_exact");
}
