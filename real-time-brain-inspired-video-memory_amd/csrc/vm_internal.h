// Handle layouts private to libvidmem.
#pragma once
#include "vm_common.h"

struct vm_memory {
    vm_ctx *ctx;
    int64_t cap;       // rows
    int D;             // multiple of 128
    int dtype;         // vm_dtype
    int ring;          // 1: overwrite oldest
    uint16_t *rows;    // [cap_pad, D] 16-bit
    double *norm64;    // [cap_pad] exact reference norm of each stored row
    float *rnorm32;    // [cap_pad] 1/norm (0 for a zero row) for the fp32 scan
    int64_t *d_total;  // device: rows appended so far (drives slots under graph replay); 64 bytes, see VM_GSTATE_*
    int64_t h_total;   // host mirror
    // grouped memories only (vm_memory_create_grouped; null otherwise)
    int64_t *gkey;     // [cap_pad] group key of each slot (a plain append stores -1 - row id)
    int64_t *gord;     // [cap_pad] group ordinal of each slot: groups ever opened before this row's group, so equal
                       // ordinals = one group and ordinals rise by 0 or 1 from each row id to the next
    // tagged memories only (vm_memory_create_tagged; null otherwise)
    int64_t *tag;      // [cap_pad] tag of each slot (INT64_MIN for a row appended without one)
};

// The 64-byte device block d_total points to: [0] row count, then the grouped append's state (zeroed with the row count
// by vm_memory_reset, so a reset also forgets the open group), then [4] the certificate's domain word (bf16 memories):
// nonzero once a row was appended whose norm lies outside the certificate's domain (topk_common.h cert_norm_outside).
// The word is STICKY: the appends set it (memory.hip, novelty.hip), only vm_memory_reset clears it; an erase or a ring
// overwrite that removes the offending row leaves it set (the searches stay exact, at exhaustive cost, until a reset),
// and a restore rebuilds it because it appends.  The bf16 searches read it where they would use cert_eps.
enum { VM_GSTATE_GROUPS = 1, VM_GSTATE_LAST_KEY = 2, VM_GSTATE_OPEN = 3, VM_GSTATE_OUTSIDE = 4 };

// Logical view of the (ring) row store for a device-side row count: searchable rows n, physical slot of the oldest
// row (head), row id of the oldest row (base).  Row of age order o (0 = oldest) sits in slot (o + head) % cap.
struct RingView {
    int64_t n, head, base, cap;
};
__host__ __device__ inline RingView ring_view(int64_t total, int64_t cap, int ring) {
    RingView v;
    v.cap = cap;
    if (ring && total > cap) {
        v.n = cap;
        v.head = total % cap;
        v.base = total - cap;
    } else {
        v.n = total < cap ? total : cap;
        v.head = 0;
        v.base = 0;
    }
    return v;
}
// physical slot of the row of age order o (0 <= o < v.n)
__host__ __device__ inline int64_t slot_of(const RingView &v, int64_t o) {
    const int64_t p = o + v.head;
    return p >= v.cap ? p - v.cap : p;
}

// age order (0 = oldest) of the live row in physical slot p
__host__ __device__ inline int64_t order_of(const RingView &v, int64_t p) {
    const int64_t o = p - v.head;
    return o < 0 ? o + v.cap : o;
}

// tagged memories: a row is in a query's scope when its tag lies in the inclusive range [lo, hi]
__host__ __device__ inline bool in_scope(int64_t tag, int64_t lo, int64_t hi) { return lo <= tag && tag <= hi; }

// Row masks (include/vidmem.h vm_topk_cosine_masked): n_masks arrays of W 32-bit words, bit s & 31 of word s >> 5 = the
// row in physical slot s.  index: null (one mask for every query, or mask q for query q) or the mask each query names.
struct MaskSel {
    const uint32_t *words;
    const int32_t *index;
    int n_masks;
    int64_t W;
};
// W of a memory: one bit per slot, in whole 64-bit pieces
inline int64_t mask_words(const vm_memory *m) { return (m->cap + 63) / 64 * 2; }
// The rules of a mask operand for Q queries, the same in every search that takes one.  The scans address a mask halfword
// by a 32-bit byte offset from `masks` (MaskScan::tile_bits, MixScan::tile_bits): at most 2^30 words of masks.  The masked
// search reports a misaligned or miscounted operand with its other arguments and uses the word limit alone.
inline int mask_limit_check(const vm_memory *m, int n_masks, const char *who) {
    if ((int64_t)n_masks * mask_words(m) > ((int64_t)1 << 30))
        return vm_fail(m->ctx, VM_ERR_UNSUPPORTED, "%s: more than 2^30 words of masks", who);
    return VM_OK;
}
inline int mask_operand_check(const vm_memory *m, const uint32_t *masks, int n_masks, const int32_t *mask_index, int Q,
                              const char *who) {
    if ((uintptr_t)masks & 3) return vm_fail(m->ctx, VM_ERR_INVALID, "%s: masks must be 4-byte aligned", who);
    if (n_masks < 1 || !(mask_index || n_masks == 1 || n_masks == Q))
        return vm_fail(m->ctx, VM_ERR_INVALID, "%s: %d masks for %d queries need a mask_index", who, n_masks, Q);
    return mask_limit_check(m, n_masks, who);
}
// word offset of query q's mask, -1 = the empty mask (an index outside [0, n_masks))
__host__ __device__ inline int64_t mask_offset(const MaskSel &ms, int q) {
    const int64_t i = ms.index ? ms.index[q] : (ms.n_masks == 1 ? 0 : q);
    return i < 0 || i >= ms.n_masks ? -1 : i * ms.W;
}
// whether the mask at word offset off (-1: empty) selects physical slot p; a consumer tests p for liveness itself
__host__ __device__ inline bool mask_selects(const uint32_t *words, int64_t off, int64_t p) {
    return off >= 0 && ((words[off + (p >> 5)] >> (p & 31)) & 1u);
}

// ---- row predicates -----------------------------------------------------------------------------------------
// What "the row in physical slot p counts for query q" means, as a type handed to a kernel by value: always (NoScope), the
// tag range of vm_topk_cosine_scoped (TagScope), the bit mask of vm_topk_cosine_masked (MaskScope), the row-id span of
// vm_topk_cosine_span (RowSpan, below them).  A model has
// `static constexpr bool scoped`, `Q at(int q) const` (what is per query, read once) and, when scoped, `bool
// Q::in(int64_t p) const`; every use sits under `if constexpr (P::scoped)`, so a NoScope instantiation carries nothing
// of it.  A consumer tests p for liveness itself.  The redo scans take one (topk_exact.hip, topk_group_parts.h), the
// grouped finalize another, and the host drivers pass them through (topk_scope_select.h, topk_group_parts.h).
struct NoScope {
    static constexpr bool scoped = false;
    struct Q {};
    __device__ __forceinline__ Q at(int) const { return {}; }
};
struct TagScope {
    static constexpr bool scoped = true;
    const int64_t *tag, *lo, *hi;
    struct Q {
        const int64_t *tag;
        int64_t lo, hi;
        __device__ __forceinline__ bool in(int64_t p) const { return in_scope(tag[p], lo, hi); }
    };
    // The scopes are read through the constant address space (no kernel writes them).  The pointers arrive inside a
    // by-value struct; the compiler does not prove the memory behind a pointer it loaded itself unwritten, as it does for a
    // __restrict__ kernel argument, and the uniform loads lo[q] / hi[q] would be vector loads into six VGPRs, not scalar
    // ones.
    __device__ __forceinline__ Q at(int q) const {
        typedef const __attribute__((address_space(4))) int64_t *scalar_ptr;
        return {tag, ((scalar_ptr)lo)[q], ((scalar_ptr)hi)[q]};
    }
};
struct MaskScope {
    static constexpr bool scoped = true;
    MaskSel ms;
    struct Q {
        const uint32_t *words;
        int64_t off;
        __device__ __forceinline__ bool in(int64_t p) const { return mask_selects(words, off, p); }
    };
    __device__ __forceinline__ Q at(int q) const { return {ms.words, mask_offset(ms, q)}; }
};

// The row-id span [row_lo, row_hi] of vm_topk_cosine_span as inclusive bounds on the AGE ORDER, clamped to the live rows
// [0, rv.n): ids below the oldest row, at or past the row count, or negative name no row.  lo > hi (here 1, 0): the span
// is empty or holds no live row.  No sum or difference leaves the live ids, so INT64_MIN / INT64_MAX are safe bounds.
struct OrderSpan {
    int64_t lo, hi;
};
__host__ __device__ inline OrderSpan order_span(const RingView &rv, int64_t row_lo, int64_t row_hi) {
    const int64_t first = rv.base, last = rv.base + rv.n - 1;
    const int64_t lo = row_lo > first ? row_lo : first, hi = row_hi < last ? row_hi : last;
    if (lo > hi) return {1, 0};
    return {lo - first, hi - first};
}
// The span predicate: slot p counts for query q when the age order of its row lies within the query's bounds.  The one
// predicate that reads no memory per row: at(q) reads the two bounds and the row count once - through the constant
// address space, for TagScope's reason - and in(p) is arithmetic on the slot.
struct RowSpan {
    static constexpr bool scoped = true;
    const int64_t *lo, *hi, *d_total;
    int64_t cap;
    int ring;
    struct Q {
        RingView rv;
        int64_t lo, hi;  // age orders
        __device__ __forceinline__ bool in(int64_t p) const {
            const int64_t o = order_of(rv, p);
            return lo <= o && o <= hi;
        }
    };
    __device__ __forceinline__ Q at(int q) const {
        typedef const __attribute__((address_space(4))) int64_t *scalar_ptr;
        const RingView rv = ring_view(((scalar_ptr)d_total)[0], cap, ring);
        const OrderSpan s = order_span(rv, ((scalar_ptr)lo)[q], ((scalar_ptr)hi)[q]);
        return {rv, s.lo, s.hi};
    }
};

// grouped memories: the live rows + the ordinal of the oldest live group + the number of live groups, from the device
// counters.  Groups are runs of equal ordinals (gord above), so live group g = ordinal - ord0, 0 <= g < ng.
struct GroupView {
    RingView rv;
    int64_t ord0, ng;
};
__device__ __forceinline__ GroupView group_view(const RingView &rv, const int64_t *gord) {
    GroupView g;
    g.rv = rv;
    g.ord0 = 0;
    g.ng = 0;
    if (rv.n > 0) {
        g.ord0 = gord[rv.head];
        g.ng = gord[slot_of(rv, rv.n - 1)] - g.ord0 + 1;
    }
    return g;
}
__device__ __forceinline__ GroupView group_view(const int64_t *d_total, int64_t cap, int ring, const int64_t *gord) {
    return group_view(ring_view(*d_total, cap, ring), gord);
}

// The rows whose every score the cut cascade keeps in its first, DENSE pass: the NEWEST stored rows (at most 4,095 of
// them, a whole number of 256-row panels plus the ragged end).  New rows are what a video's current frames resemble
// most - a scene lasts thousands of frames - so the first cut is high and the later passes emit little; with the
// physically first rows as the dense set, a growing (non-ring) memory whose newest few thousand rows all beat the cut of
// the old ones overflowed every query's candidate buffer in the last pass and sent the whole batch to the exhaustive
// redo (correct, 1 s instead of 1 ms: found by the extractor bench leg on a clip processed twice).
// Physical slots [d0, d1); the later passes scan [0, n) in physical order and skip these.
struct DenseRange {
    int64_t d0, d1;
};
__host__ __device__ inline DenseRange dense_newest(const RingView &rv) {
    const int64_t end = rv.head ? rv.head : rv.n;   // physical end (exclusive) of the newest rows
    const int64_t e_al = end & ~(int64_t)255;
    DenseRange r;
    if (e_al >= 3840) {
        r.d0 = e_al - 3840;
        r.d1 = end;
    } else {   // fewer than 15 panels before the end: the physically first rows (they contain the newest ones)
        r.d0 = 0;
        r.d1 = rv.n < 4095 ? rv.n : 4095;
    }
    return r;
}

// ---- exhaustive redo (topk_exact.hip), shared by the row, grouped and scoped searches -------------------------------
// row blocks of a redo scan that scores `chunk` rows per selection pass: the one definition of nblk
int vm_topk_redo_blocks(const vm_memory *m, int chunk);
// rows scored per selection pass by the redo scan of the row search and of the scoped search
constexpr int VM_REDO_CHUNK = 2048, VM_REDO_CHUNK_SCOPED = 1024;
// The redo scan of rows: for every flagged query, block b of nblk scores its slice of age orders exactly and leaves the
// slice's stable top-k in part_s / part_o [nblk][Q][k].  P = a row predicate (above): NoScope scores every live row in
// chunks of VM_REDO_CHUNK, nblk = vm_topk_redo_blocks(m, VM_REDO_CHUNK); a scoped P only the rows it admits, in chunks of
// VM_REDO_CHUNK_SCOPED, nblk = vm_topk_redo_blocks(m, VM_REDO_CHUNK_SCOPED).  Instantiated in topk_exact.hip for the four
// predicates.  vm_topk_redo_merge follows.
template <class P>
int vm_topk_redo_scan(vm_memory *m, const void *queries, int Q, int k, const P &pred, const int32_t *flags, int nblk,
                      double *part_s, int64_t *part_o, hipStream_t st);
// Merge of the redo scans' slice winners, part_s / part_o [nblk][Q][k] = {score, age order}, for the flagged queries:
// stable top-k, score mapping, min_score, row id = (base + order) * row_stride + row_offset.  gkey / out_keys: null, or
// the grouped search's key column and key output.
int vm_topk_redo_merge(vm_memory *m, const double *part_s, const int64_t *part_o, int nblk, int Q, int k,
                       const int32_t *flags, int use_min, double min_score, int score_mode, int64_t row_stride,
                       int64_t row_offset, double *out_scores, int64_t *out_rows, const int64_t *gkey,
                       int64_t *out_keys, hipStream_t st);

// ---- emit-only many-query scan (topk_emit.hip), driven by topk.hip ---------------------------------------------
constexpr int VM_EMIT_CAP = 4096;  // candidate slots per query; more -> the query is marked for the exhaustive redo
bool vm_topk_emit_supported(const vm_memory *m, int Q, int KL);
size_t vm_topk_emit_workspace_bytes(int q_pad);
int vm_topk_emit_scan(vm_memory *m, const void *queries, int Q, int q_thr, const float *thr_s, const int *thr_o,
                      int *cand_cnt, float *cand_s, int *cand_o, int64_t row_begin, int64_t row_limit, hipStream_t st);
int vm_topk_emit_compact(vm_memory *m, int Q, int KL, int *cand_cnt, float *cand_s, int *cand_o, float *part_s,
                         int *part_o, int *mark, float *cut_s, int *cut_o, int seed, hipStream_t st);
// ---- GEMM-class scan for very many queries (topk_gscan.hip), reached through vm_topk_emit_scan ---------------------
bool vm_topk_gscan_supported(const vm_memory *m, int Q, int64_t rows);
int vm_topk_gscan(vm_memory *m, const void *queries, int Q, int q_thr, const float *thr_s, const int *thr_o,
                  int *cand_cnt, float *cand_s, int *cand_o, int64_t row_begin, int64_t row_limit, hipStream_t st);
