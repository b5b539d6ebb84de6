// The interface of the select stage over one fp32 key per (query, physical slot), key 0 = "not a candidate": the cut from a
// strided sample, the parallel compaction of every slot at or above it and the block-wide selection of the best M + 1.
// Written for the scoped search (topk_scope.hip: key 0 = out of scope) and shared, unchanged, with the clip search
// (topk_clip.hip: key 0 = no valid, in-scope window that could be a peak starts in the slot), the masked, the span and the
// mixed search (topk_mask.hip, topk_span.hip, topk_mix.hip).  The scoped, the masked and the span search also share what
// follows the selection: the exact finalize with the gap certificate, the workspace plan and the host driver (RowCall,
// key_image_topk, key_image_exact): a search brings its scan policy and its row predicate (vm_internal.h), nothing else.
// The kernels and their launches are compiled once, in topk_key_image.hip; here are the constants, the two
// structs and the declarations another unit needs, and the host templates that have to see a scan policy or a predicate.
// topk_group_parts.h reuses constant names with other values (SEL_CAP): no unit may include both headers.
#pragma once
#include "topk_select.h"
#include "topk_tile_scan.h"  // TS_THREADS: the plan sizes the scan's grid

constexpr int SEL_CAP = 8192;    // rows at or above the cut a query keeps; more -> VM_FLAG_OVERFLOW
constexpr int SF_THREADS = 256;  // finalize
constexpr int SCMAX = 128;       // candidates per query kept by the select (M + 1 <= 81)
constexpr int SKMAX = 64;

// ---- host: the workspace ---------------------------------------------------------------------------------------
// what the select stage reads of a plan: the geometry, the key image's row stride and where its arrays lie
struct SelectPlan : TopkGeom {
    int64_t fstride;
    size_t off_co, off_ck, off_cn, off_cut, off_cc, off_cbuf;
};
// the workspace of a search that keeps F[q][slot] at offset 0, selects and finalizes (scoped, masked, span, mixed)
struct SPlan : SelectPlan {
    size_t off_flags, off_ps, off_po, total;
};
SPlan vm_key_image_plan(const vm_memory *m, int Q, int k);

// what every entry point of a row search is called with, past the operands of its predicate
struct RowCall {
    const void *queries;
    int Q, k, use_min;
    double min_score;
    int score_mode;
    int64_t row_stride, row_offset;
    double *out_scores;
    int64_t *out_rows;
    int32_t *out_uncertified, *out_query_flags;  // null in the exhaustive-only entry points
    char *ws;
    hipStream_t stream;
};

// ---- host: the launches (topk_key_image.hip) -------------------------------------------------------------------
// cut -> compact -> select over the key image F [Q][p.fstride]: per key row the best p.M + 1 slots by (key desc, age
// order asc) into cand_o / cand_k / cand_n at the plan's offsets in ws
int vm_key_image_select(vm_memory *m, const SelectPlan &p, const uint32_t *F, int Q, char *ws, hipStream_t st);
// the exact finalize of the candidates with the gap certificate, for the memory's dtype
int vm_key_image_finalize(vm_memory *m, const SPlan &p, const RowCall &c);
// flags[0, n) = 1: every query (clip) is flagged, which is what makes a redo the exhaustive-only entry point
int vm_fill_flags(vm_memory *m, int32_t *flags, int n, hipStream_t st);

// ---- host: the one driver of those searches ----------------------------------------------------------------
// redo: flagged queries scored exhaustively over the rows pred admits, then the one merge of every redo
template <class P>
int key_image_redo(vm_memory *m, const SPlan &p, const RowCall &c, const P &pred) {
    vm_prof_scope prof(m->ctx, VM_PROF_TOPK_EXACT, c.stream);
    const int32_t *flags = (const int32_t *)(c.ws + p.off_flags);
    double *part_s = (double *)(c.ws + p.off_ps);
    int64_t *part_o = (int64_t *)(c.ws + p.off_po);
    if (int rc = vm_topk_redo_scan(m, c.queries, c.Q, c.k, pred, flags, p.nblk, part_s, part_o, c.stream)) return rc;
    return vm_topk_redo_merge(m, part_s, part_o, p.nblk, c.Q, c.k, flags, c.use_min, c.min_score, c.score_mode,
                              c.row_stride, c.row_offset, c.out_scores, c.out_rows, nullptr, nullptr, c.stream);
}

// scan -> cut -> compact -> select -> finalize -> redo.  Scan: the tile-scan policy that writes the key image (its Args
// have fstride and F, which are the plan's and filled in here); pred: the same row set for the redo.
template <int DT, class Scan, class P>
int key_image_topk(vm_memory *m, const RowCall &c, typename Scan::Args a, const P &pred) {
    const SPlan p = vm_key_image_plan(m, c.Q, c.k);
    uint32_t *F = (uint32_t *)c.ws;
    {
        vm_prof_scope prof(m->ctx, VM_PROF_TOPK_SCAN, c.stream);
        a.fstride = p.fstride;
        a.F = F;
        const int rc = vm_tile_scan<DT, Scan>(m, p, c.queries, c.Q, a, c.stream);
        if (rc != VM_OK) return rc;
    }
    {
        vm_prof_scope prof(m->ctx, VM_PROF_TOPK_FINALIZE, c.stream);
        if (int rc = vm_key_image_select(m, p, F, c.Q, c.ws, c.stream)) return rc;
        if (int rc = vm_key_image_finalize(m, p, c)) return rc;
    }
    return key_image_redo(m, p, c, pred);
}

// the exhaustive-only entry point: every query flagged, then the redo
template <class P>
int key_image_exact(vm_memory *m, const RowCall &c, const P &pred) {
    const SPlan p = vm_key_image_plan(m, c.Q, c.k);
    if (int rc = vm_fill_flags(m, (int32_t *)(c.ws + p.off_flags), c.Q, c.stream)) return rc;
    return key_image_redo(m, p, c, pred);
}
