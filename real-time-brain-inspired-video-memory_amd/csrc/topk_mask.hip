// Masked cosine top-k: the k best rows among those a device BIT MASK selects (include/vidmem.h vm_topk_cosine_masked),
// and the two device-side builders of such masks.  The row set is an operand: one bit per physical slot, built on the
// host or on the device, combined with & | ~ by the caller, named per query.  Generalises the one predicate shape of the
// scoped search (topk_scope.hip: one inclusive tag range per query) to any set: a metadata filter, the hits of another
// search, an exclusion, a union of windows.
//
// The scoped search with another predicate, and built from the same parts:
//   scan     : topk_tile_scan.h under the MaskScan policy below.  Per 16-row tile the wave first reads the tile's 16 mask
//              bits of each of its queries (2 bytes per query, against the 128 bytes of tags of the scoped pre-test); a
//              tile no query selects a live row of is skipped WITHOUT reading its rows and only zeroes its keys.
//              Otherwise fp32 MFMA scores, F[q][slot] = okey32(score) for a selected live row, 0 for any other
//   select   : topk_key_image.hip, through topk_scope_select.h: the best M + 1 selected rows by (fp32 key desc, age order
//              asc)
//   finalize : topk_key_image.hip's scope_finalize_kernel: nothing in it is specific to scopes.  Certified
//              when the mask selects at most M rows, or when the exact k-th score clears the (M+1)-th SELECTED fp32
//              score / ||q|| by cert_eps(D), strictly.  Unselected rows have key 0 and never reach the certificate
//   redo     : vm_topk_redo_scan under the MaskScope predicate (vm_internal.h, topk_exact.hip), then vm_topk_redo_merge
// A bit whose slot holds no live row is ignored everywhere: the scan and the redo visit live slots only.
// Every launch reads the row count from the device and sizes its grid from the capacity: capturable.
#include "topk_scope_select.h"
#include "topk_tile_scan.h"

namespace {

// ---- scan --------------------------------------------------------------------------------------------------
// The masked policy of the tile scan: four keys per lane, F[q * fstride + slot] = the order-preserving key of the fp32
// score, or 0 when the query's mask does not select the slot or the slot is past the live rows.  A tile's 16 bits are
// halfword tile & 1 of word tile >> 1 of the mask: halfword `tile` from the mask's first word (little endian).
struct MaskScan {
    struct Args {
        MaskSel ms;
        int64_t fstride;
        uint32_t *F;
    };
    template <int QT>
    struct QState {
        int off[QT * 16];  // word offset of the query's mask, -1 = the empty mask (also: the query is past Q)
    };
    struct View {};
    template <class QS>
    static __device__ __forceinline__ void load_query(QS &qs, const Args &a, int i, int q, bool live) {
        qs.off[i] = live ? (int)mask_offset(a.ms, q) : -1;
    }
    static __device__ __forceinline__ View view(const Args &, const RingView &) { return {}; }
    // the 16 bits of `tile` in the mask at word offset off, the slots at and past n cleared
    static __device__ __forceinline__ uint32_t tile_bits(const Args &a, int off, const TileLane &l) {
        if (off < 0) return 0u;
        // the tile is the same in every lane of a wave: what depends on it alone is scalar, so that nothing of it stays in
        // VGPRs across the MFMA loop (without this: 84 VGPRs at QT = 2, against ScopeScan's 80)
        const int tile = __builtin_amdgcn_readfirstlane((int)l.tile);
        const int64_t left = l.n - (int64_t)tile * 16;  // >= 1: the scan visits tiles that hold a live slot
        const uint32_t live = left < 16 ? (1u << left) - 1u : 0xffffu;
        // a 32-bit byte offset from the masks' base (the host refuses more than 2^30 words of masks): one address VGPR
        const uint32_t byte = (uint32_t)off * 4u + (uint32_t)tile * 2u;
        const uint32_t b = *reinterpret_cast<const uint16_t *>(reinterpret_cast<const char *>(a.ms.words) + byte) & live;
        return b;
    }
    template <int QT>
    static __device__ __forceinline__ bool skip_tile(const QState<QT> &qs, const Args &a, const TileLane &l) {
        // lane i < QT * 16 reads the tile's bits of block query i; wave-uniform: some query selects some live row
        const uint32_t b = l.lane < QT * 16 ? tile_bits(a, qs.off[l.lane], l) : 0u;
        if (__ballot(b != 0u) != 0ull) return false;
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
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const int q = l.q0 + 16 * t + l.r16;
            if (q >= l.Q) continue;
            const uint32_t b = tile_bits(a, qs.off[16 * t + l.r16], l) >> (4 * l.h);  // the lane's four slots
            uint32_t key[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) key[j] = ((b >> j) & 1u) ? okey32(s[t][j]) : 0u;
            *reinterpret_cast<uint4 *>(a.F + (size_t)q * a.fstride + l.p0()) = make_uint4(key[0], key[1], key[2], key[3]);
        }
    }
};

// ---- builders ----------------------------------------------------------------------------------------------
// Thread = one entry of row_ids: the bit of a live row's slot is ORed into the mask (the result does not depend on the
// order of the atomics).  -1, an id that is not row * stride + offset, and a row that is not live are skipped.
__global__ void __launch_bounds__(256)
    mask_from_rows_kernel(const int64_t *__restrict__ row_ids, int64_t n, int64_t row_stride, int64_t row_offset,
                          const int64_t *__restrict__ d_total, int64_t cap, int ring, uint32_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t id = row_ids[i];
    if (id < 0) return;
    const int64_t d = id - row_offset;
    if (d < 0 || d % row_stride != 0) return;
    const int64_t r = d / row_stride;
    const RingView rv = ring_view(*d_total, cap, ring);
    if (r < rv.base || r >= rv.base + rv.n) return;
    const int64_t s = r % cap;  // = slot_of(rv, r - rv.base): below W * 32
    atomicOr(out + (s >> 5), 1u << (s & 31));
}

// Thread = one slot, a wave = two words of the mask; the grid covers all W * 32 slots, so every word is written and a
// slot that holds no live row gives 0.
__global__ void __launch_bounds__(256)
    mask_from_scopes_kernel(const int64_t *__restrict__ tag, const int64_t *__restrict__ scope_lo,
                            const int64_t *__restrict__ scope_hi, int n_ranges, const int64_t *__restrict__ d_total,
                            int64_t cap, int ring, int64_t W, uint32_t *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= W * 32) return;  // wave-uniform: W * 32 is a multiple of 64
    const int64_t n = ring_view(*d_total, cap, ring).n;
    bool in = false;
    if (p < n) {
        const int64_t tg = tag[p];
        for (int i = 0; i < n_ranges; ++i) in |= in_scope(tg, scope_lo[i], scope_hi[i]);
    }
    const unsigned long long b = __ballot(in);
    const int lane = threadIdx.x & 63;
    if (lane == 0) out[p >> 5] = (uint32_t)b;
    if (lane == 32) out[p >> 5] = (uint32_t)(b >> 32);
}

// ---- host --------------------------------------------------------------------------------------------------
// the mask operand's rules are vm_internal.h's; a misaligned or miscounted one is a bad argument here, with the others
int mask_check(vm_memory *m, const RowCall &c, const uint32_t *masks, int n_masks, const int32_t *mask_index,
               size_t workspace_bytes, const char *who) {
    const bool ok = c.queries && masks && c.out_scores && c.out_rows && c.Q > 0 && n_masks > 0 &&
                    (mask_index || n_masks == 1 || n_masks == c.Q) && !((uintptr_t)masks & 3);
    if (ok)
        if (int rc = mask_limit_check(m, n_masks, who)) return rc;
    return vm_topk_check(m, nullptr, ok, c.queries, c.k, SKMAX, VM_ERR_INVALID, c.score_mode, c.ws, workspace_bytes,
                         vm_key_image_plan(m, c.Q, c.k).total, who);
}

// both entry points: the fast form (topk_scope_select.h key_image_topk under MaskScan; the scoped search's workspace, the
// same stages over the same key image) or the exhaustive one
int mask_entry(vm_memory *m, const RowCall &c, const uint32_t *masks, int n_masks, const int32_t *mask_index,
               size_t workspace_bytes, bool exact, const char *who) {
    if (!m) return VM_ERR_INVALID;
    if (int rc = mask_check(m, c, masks, n_masks, mask_index, workspace_bytes, who)) return rc;
    const MaskScope ms = {{masks, mask_index, n_masks, mask_words(m)}};
    if (exact) return key_image_exact(m, c, ms);
    return vm_by_dtype(m, [&](auto dt) {
        return key_image_topk<decltype(dt)::value, MaskScan>(m, c, {ms.ms, 0, nullptr}, ms);
    });
}

}  // namespace

extern "C" int64_t vm_memory_mask_words(const vm_memory *m) { return m ? mask_words(m) : 0; }

extern "C" size_t vm_topk_masked_workspace_bytes(const vm_memory *m, int Q, int k) {
    if (!m || Q <= 0 || k <= 0 || k > SKMAX) return 0;
    return vm_key_image_plan(m, Q, k).total;
}

extern "C" int vm_topk_cosine_masked(vm_memory *m, const void *queries, int Q, int k, const uint32_t *masks,
                                     int n_masks, const int32_t *mask_index, int use_min_score, double min_score,
                                     int score_mode, int64_t row_stride, int64_t row_offset, double *out_scores,
                                     int64_t *out_rows, int32_t *out_uncertified, int32_t *out_query_flags,
                                     void *workspace, size_t workspace_bytes, void *stream) {
    const RowCall c = {queries,    Q,          k,          use_min_score, min_score,       score_mode,
                       row_stride, row_offset, out_scores, out_rows,      out_uncertified, out_query_flags,
                       (char *)workspace, (hipStream_t)stream};
    return mask_entry(m, c, masks, n_masks, mask_index, workspace_bytes, false, "vm_topk_cosine_masked");
}

extern "C" int vm_topk_cosine_masked_exact(vm_memory *m, const void *queries, int Q, int k, const uint32_t *masks,
                                           int n_masks, const int32_t *mask_index, int use_min_score, double min_score,
                                           int score_mode, int64_t row_stride, int64_t row_offset, double *out_scores,
                                           int64_t *out_rows, void *workspace, size_t workspace_bytes, void *stream) {
    const RowCall c = {queries,    Q,          k,          use_min_score, min_score, score_mode,
                       row_stride, row_offset, out_scores, out_rows,      nullptr,   nullptr,
                       (char *)workspace, (hipStream_t)stream};
    return mask_entry(m, c, masks, n_masks, mask_index, workspace_bytes, true, "vm_topk_cosine_masked_exact");
}

extern "C" int vm_mask_from_rows(vm_memory *m, const int64_t *row_ids, int64_t n, int64_t row_stride,
                                 int64_t row_offset, int clear_first, uint32_t *out_mask, void *stream) {
    if (!m) return VM_ERR_INVALID;
    vm_ctx *ctx = m->ctx;
    if (!out_mask || ((uintptr_t)out_mask & 3) || n < 0 || (n > 0 && !row_ids) || row_stride < 1)
        return vm_fail(ctx, VM_ERR_INVALID, "vm_mask_from_rows: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (clear_first) VM_HIP(ctx, hipMemsetAsync(out_mask, 0, (size_t)mask_words(m) * 4, st));
    if (n == 0) return VM_OK;
    mask_from_rows_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(row_ids, n, row_stride, row_offset, m->d_total,
                                                                     m->cap, m->ring, out_mask);
    VM_LAUNCH_CHECK(ctx);
    return VM_OK;
}

extern "C" int vm_mask_from_scopes(vm_memory *m, const int64_t *scope_lo, const int64_t *scope_hi, int n_ranges,
                                   uint32_t *out_mask, void *stream) {
    if (!m) return VM_ERR_INVALID;
    vm_ctx *ctx = m->ctx;
    if (!m->tag) return vm_fail(ctx, VM_ERR_INVALID, "vm_mask_from_scopes: the memory is not tagged");
    if (!out_mask || ((uintptr_t)out_mask & 3) || n_ranges < 0 || (n_ranges > 0 && (!scope_lo || !scope_hi)))
        return vm_fail(ctx, VM_ERR_INVALID, "vm_mask_from_scopes: bad arguments");
    const int64_t W = mask_words(m);
    mask_from_scopes_kernel<<<(unsigned)((W * 32 + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        m->tag, scope_lo, scope_hi, n_ranges, m->d_total, m->cap, m->ring, W, out_mask);
    VM_LAUNCH_CHECK(ctx);
    return VM_OK;
}
