// Novelty-gated append: a batch row is stored only when nothing resembles it (include/vidmem.h
// vm_memory_append_novel).  The reference has no counterpart: it stores one text embedding per chunk
// (src/components/neo4j_handler.py:229-242); the decision rule is the build's own, taken on the reference cosine of
// topk_common.h bit for bit.
//
// In row order: row l is dropped when the caller's search already found a stored row above the threshold
// (known_score > tau), or when an EARLIER KEPT row of the batch scores above it; otherwise it is kept and appended as
// vm_memory_append[_grouped|_tagged] would append the sub-batch of kept rows.  Nothing scans the memory, nothing is
// read on the host: four launches (five on a grouped memory), each sized from B, the row count read from the device.
//   1 norms    norm64 of every batch row, once
//   2 pairs    thread = one pair (l, i), i < l: exact cosine; one __ballot of a wave's 64 consecutive l = one word of the
//              bit matrix A[i][l / 64] = "row l is too close to the earlier row i" (plain vector store, no atomics)
//   3 resolve  ONE wave: lane w holds word w of the suppressed set; greedy in row order, 64 rows at a time
//   4 append   one block per batch row: a kept row is copied to its slot with its norm and tag, a dropped row looks up the
//              row that suppressed it
//   5 groups   keys and ordinals over the kept rows (grouped memories only)
#include "topk_common.h"
#include "vm_internal.h"

#include <climits>

namespace {

constexpr int NOVEL_MAX_B = 4096;   // 64 lanes x 64 bits of the single-wave resolve
constexpr int NOVEL_MAX_D = 16384;  // one row in LDS (pairs kernel)

// What the resolve hands to the kernels behind it (head of the workspace).
struct NovelHeader {
    uint64_t kept[64];    // bit l % 64 of word l / 64: row l is kept
    uint64_t known[64];   // ... row l was suppressed by the caller's known_row
    int32_t prefix[64];   // kept rows in the words before word w
    int64_t total0;       // device row count before the call
    int32_t count;        // kept rows of this call
    int32_t pad_;
};
constexpr size_t NOVEL_HEADER_BYTES = 2048;
static_assert(sizeof(NovelHeader) <= NOVEL_HEADER_BYTES, "header layout");

struct NovelWorkspace {
    NovelHeader *hdr;
    double *norm;      // [B]
    uint64_t *A;       // [B, W]
};
inline size_t novel_ws_bytes(int B) {
    const size_t W = (size_t)(B + 63) / 64;
    return NOVEL_HEADER_BYTES + vm_align_up((size_t)B * 8, 256) + (size_t)B * W * 8;
}
inline NovelWorkspace novel_ws_carve(void *ws, int B) {
    char *p = (char *)ws;
    NovelWorkspace w;
    w.hdr = (NovelHeader *)p;
    w.norm = (double *)(p + NOVEL_HEADER_BYTES);
    w.A = (uint64_t *)(p + NOVEL_HEADER_BYTES + vm_align_up((size_t)B * 8, 256));
    return w;
}

// Word w of A[i] holds a bit of some row l > i (and is therefore written by the pairs kernel) iff this is true.
__device__ __forceinline__ bool word_is_live(int i, int w, int B) {
    const int last = 64 * w + 63 < B - 1 ? 64 * w + 63 : B - 1;
    return last > i;
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int lane) {   // lane is wave-uniform
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}

// rank of row i among the kept rows = kept rows before it
__device__ __forceinline__ int kept_rank(const NovelHeader *h, int i) {
    return h->prefix[i >> 6] + __popcll(h->kept[i >> 6] & ((1ull << (i & 63)) - 1));
}

// 1. One thread per batch row: the reference norm (memory_append_kernel's, computed once for the pairs and the append).
template <int DT>
__global__ void __launch_bounds__(64) novel_norm_kernel(const uint16_t *__restrict__ src, int B, int D,
                                                        double *__restrict__ norm) {
    const int l = blockIdx.x * 64 + threadIdx.x;
    if (l < B) norm[l] = __dsqrt_rn(ref_sumsq<DT>(src + (size_t)l * D, D));
}

// 2. grid (ceil(B / 256), B): block (t, i) scores rows l = 256 t + tid against the EARLIER row i, which sits in LDS.
template <int DT>
__global__ void __launch_bounds__(256) novel_pairs_kernel(const uint16_t *__restrict__ src, int B, int D, int W,
                                                          const double *__restrict__ norm, double tau,
                                                          uint64_t *__restrict__ A) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint16_t *ql = reinterpret_cast<uint16_t *>(smem);
    const int i = blockIdx.y;
    const int l0 = blockIdx.x * 256;
    const int last = l0 + 255 < B - 1 ? l0 + 255 : B - 1;
    if (last <= i) return;   // no row of this tile comes after row i (uniform)
    const uint16_t *qv = src + (size_t)i * D;
    for (int c = threadIdx.x; c < D / 8; c += 256)
        reinterpret_cast<uint4 *>(ql)[c] = reinterpret_cast<const uint4 *>(qv)[c];
    __syncthreads();
    const int l = l0 + threadIdx.x;
    bool close = false;
    if (l < B && l > i) {
        const double dot = ref_dot<DT>(ql, src + (size_t)l * D, D);
        close = ref_cosine(dot, norm[l], norm[i]) > tau;   // strict, like passes_min
    }
    const uint64_t word = __ballot(close);
    const int w = l >> 6;
    if ((threadIdx.x & 63) == 0 && w < W) A[(size_t)i * W + w] = word;
}

// 3. ONE wave.  Lane w holds word w of the suppressed set, initialised from known_*.  Rows are resolved 64 at a time:
// the 64 x 64 diagonal block of A (lane b: word c of A[64 c + b]) settles the rows of word c among themselves in
// registers, then the words of the kept rows are ORed into the later lanes, eight loads in flight.  Writes the kept and
// known masks, the per-word prefix counts and the count, and moves the device row counter (the kernels behind read the
// snapshot total0, never the counter).
__global__ void __launch_bounds__(64) novel_resolve_kernel(const uint64_t *__restrict__ A, int B, int W, double tau,
                                                           const double *__restrict__ known_scores,
                                                           const int64_t *__restrict__ known_rows, int64_t known_stride,
                                                           int64_t *__restrict__ d_total, int64_t cap, int ring,
                                                           NovelHeader *__restrict__ hdr,
                                                           int32_t *__restrict__ out_count) {
    const int lane = threadIdx.x;
    uint64_t supp = 0;
    if (known_scores) {
        for (int c = 0; c < W; ++c) {
            const int i = 64 * c + lane;
            bool s = false;
            if (i < B) s = known_rows[(int64_t)i * known_stride] >= 0 && known_scores[(int64_t)i * known_stride] > tau;
            const uint64_t m = __ballot(s);
            if (lane == c) supp = m;
        }
    }
    const uint64_t known = supp;
    uint64_t kept = 0;
    auto load_diag = [&](int c) -> uint64_t {
        const int i = 64 * c + lane;
        return (c < W && i < B && word_is_live(i, c, B)) ? A[(size_t)i * W + c] : 0;
    };
    uint64_t diag = load_diag(0);
    for (int c = 0; c < W; ++c) {
        const uint64_t diag_next = load_diag(c + 1);   // does not depend on the state: in flight during this word
        const int nb = B - 64 * c < 64 ? B - 64 * c : 64;
        uint64_t cur = readlane64(supp, c);
        if (__ballot(diag != 0)) {
            for (int b = 0; b < nb; ++b) {
                const uint64_t d = readlane64(diag, b);
                if (!((cur >> b) & 1)) cur |= d;
            }
        }
        const uint64_t valid = nb == 64 ? ~0ull : (1ull << nb) - 1;
        const uint64_t keptw = ~cur & valid;
        if (lane == c) kept = keptw;
        // the kept rows of this word suppress rows of the later words (lanes c < lane < W: those words are live)
        const bool later = lane > c && lane < W;
        const uint64_t *Ac = A + (size_t)64 * c * W + (later ? lane : W - 1);
        uint64_t m = keptw;
        while (m) {
            uint64_t v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int b = m ? __builtin_ctzll(m) : -1;
                m &= m - 1;   // 0 stays 0
                v[u] = 0;
                if (later && b >= 0) v[u] = Ac[(size_t)b * W];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) supp |= v[u];
        }
        diag = diag_next;
    }
    // per-word prefix counts: inclusive scan of the popcounts over the 64 lanes
    const int mine = __popcll(kept);
    int inc = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(inc, off, 64);
        if (lane >= off) inc += v;
    }
    const int count = __shfl(inc, 63, 64);
    hdr->kept[lane] = kept;
    hdr->known[lane] = known;
    hdr->prefix[lane] = inc - mine;
    if (lane == 0) {
        const int64_t total0 = *d_total;
        hdr->total0 = total0;
        hdr->count = count;
        if (out_count) *out_count = count;
        int64_t stored = count;
        if (!ring) {   // never move the counter past the capacity (the host refuses such a call; a stale mirror may not)
            const int64_t room = cap > total0 ? cap - total0 : 0;
            if (stored > room) stored = room;
        }
        *d_total = total0 + stored;
    }
}

// 4. One block per batch row.  Kept: memory_append_kernel's body with the precomputed norm, plus the tag.  Dropped: the
// row that stands for it - its known_row, or the LOWEST kept earlier row of the batch whose word of A has its bit.
template <int DT>
__global__ void __launch_bounds__(128) novel_append_kernel(const uint16_t *__restrict__ src, int B, int D, int W,
                                                           const uint64_t *__restrict__ A,
                                                           const NovelHeader *__restrict__ hdr,
                                                           const double *__restrict__ norm,
                                                           const int64_t *__restrict__ known_rows, int64_t known_stride,
                                                           const int64_t *__restrict__ tags, uint16_t *__restrict__ rows,
                                                           double *__restrict__ norm64, float *__restrict__ rnorm32,
                                                           int64_t *__restrict__ tagcol, int64_t cap, int ring,
                                                           int32_t *__restrict__ out_keep,
                                                           int64_t *__restrict__ out_row_of, int64_t *dom) {
    __shared__ int best[2];
    const int l = blockIdx.x;
    const int w = l >> 6;
    const uint64_t bit = 1ull << (l & 63);
    const int64_t total0 = hdr->total0;
    if (hdr->kept[w] & bit) {
        const int64_t id = total0 + kept_rank(hdr, l);
        const int64_t slot = ring ? (id % cap) : id;
        if (threadIdx.x == 0) {
            if (out_keep) out_keep[l] = 1;
            if (out_row_of) out_row_of[l] = id;
        }
        if (slot >= cap) return;   // non-ring overflow is rejected on the host; never write out of bounds
        const uint4 *s4 = reinterpret_cast<const uint4 *>(src + (size_t)l * D);
        uint4 *d4 = reinterpret_cast<uint4 *>(rows + (size_t)slot * D);
        for (int c = threadIdx.x; c < D / 8; c += blockDim.x) d4[c] = s4[c];
        if (threadIdx.x == 0) {
            const double nrm = norm[l];
            norm64[slot] = nrm;
            rnorm32[slot] = nrm > 0.0 ? (float)(1.0 / nrm) : 0.0f;
            if (DT == VM_BF16 && cert_norm_outside(nrm)) *dom = 1;   // as memory_append_kernel: the sticky domain word
            if (tagcol) tagcol[slot] = tags ? tags[l] : LLONG_MIN;
        }
        return;
    }
    if (threadIdx.x == 0 && out_keep) out_keep[l] = 0;
    if (!out_row_of) return;
    if (hdr->known[w] & bit) {
        if (threadIdx.x == 0) out_row_of[l] = known_rows[(int64_t)l * known_stride];
        return;
    }
    int mine = INT_MAX;   // a thread's first hit is its lowest
    for (int i = threadIdx.x; i < l; i += 128) {
        if (((hdr->kept[i >> 6] >> (i & 63)) & 1) && (A[(size_t)i * W + w] & bit)) {
            mine = i;
            break;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(mine, off, 64);
        mine = o < mine ? o : mine;
    }
    if ((threadIdx.x & 63) == 0) best[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int i = best[0] < best[1] ? best[0] : best[1];
        out_row_of[l] = i == INT_MAX ? -1 : total0 + kept_rank(hdr, i);   // (a dropped row always has a suppressor)
    }
}

// 5. Grouped memories: memory_group_kernel's scan over the KEPT rows - a kept row opens a new group when its key differs
// from the previous KEPT row's (the first kept row: from the last key of the previous call, under the same rule).  A call
// that keeps nothing leaves the group state as it was.
__global__ void __launch_bounds__(256) novel_group_kernel(const int64_t *__restrict__ keys, int B,
                                                          const NovelHeader *__restrict__ hdr,
                                                          int64_t *__restrict__ gkey, int64_t *__restrict__ gord,
                                                          int64_t *__restrict__ state, int64_t cap, int ring) {
    __shared__ int scan[256];
    if (hdr->count == 0) return;
    const int tid = threadIdx.x;
    const int64_t total0 = hdr->total0;
    int64_t groups = state[VM_GSTATE_GROUPS];
    const int64_t last_key = state[VM_GSTATE_LAST_KEY];
    const bool open = state[VM_GSTATE_OPEN] != 0;
    int last_kept = -1;
    for (int c0 = 0; c0 < B; c0 += 256) {
        const int i = c0 + tid;
        int64_t kv = 0;
        int flag = 0, rank = 0;
        bool kept = false;
        if (i < B) {
            int w = i >> 6;
            const uint64_t kw = hdr->kept[w];
            kept = (kw >> (i & 63)) & 1;
            if (kept) {
                rank = kept_rank(hdr, i);
                kv = keys ? keys[i] : -1 - (total0 + rank);
                if (!keys) {
                    flag = 1;
                } else {
                    uint64_t m = kw & ((1ull << (i & 63)) - 1);   // the previous kept row
                    while (m == 0 && w > 0) m = hdr->kept[--w];
                    if (m == 0)
                        flag = !(open && kv == last_key);
                    else
                        flag = keys[64 * w + 63 - __builtin_clzll(m)] != kv;
                }
            }
        }
        scan[tid] = flag;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int v = tid >= off ? scan[tid - off] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        if (kept) {
            const int64_t id = total0 + rank;
            const int64_t slot = ring ? id % cap : id;
            if (slot < cap) {
                gkey[slot] = kv;
                gord[slot] = groups + scan[tid] - 1;
            }
        }
        groups += scan[255];
        __syncthreads();
    }
    if (tid == 0) {
        for (int w = (B - 1) >> 6; w >= 0 && last_kept < 0; --w) {
            const uint64_t m = hdr->kept[w];
            if (m) last_kept = 64 * w + 63 - __builtin_clzll(m);
        }
        state[VM_GSTATE_GROUPS] = groups;
        state[VM_GSTATE_LAST_KEY] = keys ? keys[last_kept] : 0;
        state[VM_GSTATE_OPEN] = keys ? 1 : 0;
    }
}

}  // namespace

extern "C" size_t vm_novelty_workspace_bytes(const vm_memory *m, int B) {
    if (!m || B <= 0 || B > NOVEL_MAX_B) return 0;
    return novel_ws_bytes(B);
}

extern "C" int vm_memory_append_novel(vm_memory *m, const void *rows, int B, double threshold,
                                      const double *known_scores, const int64_t *known_rows, int64_t known_stride,
                                      const int64_t *tags, const int64_t *keys, int32_t *out_keep, int64_t *out_row_of,
                                      int32_t *out_count, void *workspace, size_t workspace_bytes, void *stream) {
    if (!m) return VM_ERR_INVALID;
    vm_ctx *ctx = m->ctx;
    hipStream_t st = (hipStream_t)stream;
    if (B < 0 || (B > 0 && !rows)) return vm_fail(ctx, VM_ERR_INVALID, "vm_memory_append_novel: bad arguments");
    if (threshold != threshold) return vm_fail(ctx, VM_ERR_INVALID, "vm_memory_append_novel: the threshold is NaN");
    if ((known_scores == nullptr) != (known_rows == nullptr))
        return vm_fail(ctx, VM_ERR_INVALID, "vm_memory_append_novel: known_scores and known_rows go together");
    if (known_scores && known_stride < 1)
        return vm_fail(ctx, VM_ERR_INVALID, "vm_memory_append_novel: known_stride %lld", (long long)known_stride);
    if (tags && !m->tag) return vm_fail(ctx, VM_ERR_INVALID, "vm_memory_append_novel: tags on a memory that is not tagged");
    if (keys && !m->gkey) return vm_fail(ctx, VM_ERR_INVALID, "vm_memory_append_novel: keys on a memory that is not grouped");
    if (B == 0) {
        if (out_count) VM_HIP(ctx, hipMemsetAsync(out_count, 0, sizeof(int32_t), st));
        return VM_OK;
    }
    if (B > NOVEL_MAX_B)
        return vm_fail(ctx, VM_ERR_UNSUPPORTED, "vm_memory_append_novel: B=%d above %d rows per call", B, NOVEL_MAX_B);
    if (m->D > NOVEL_MAX_D) return vm_fail(ctx, VM_ERR_UNSUPPORTED, "vm_memory_append_novel: D=%d above %d", m->D, NOVEL_MAX_D);
    if (!m->ring && m->h_total + B > m->cap)
        return vm_fail(ctx, VM_ERR_NOMEM, "memory full: %lld + %d > capacity %lld", (long long)m->h_total, B,
                       (long long)m->cap);
    if (m->ring && B > m->cap) return vm_fail(ctx, VM_ERR_INVALID, "append of %d rows exceeds ring capacity", B);
    if (!workspace || workspace_bytes < novel_ws_bytes(B))
        return vm_fail(ctx, VM_ERR_NOMEM, "vm_memory_append_novel: workspace too small");
    const NovelWorkspace ws = novel_ws_carve(workspace, B);
    const int W = (B + 63) / 64;
    const int D = m->D;
    const uint16_t *src = (const uint16_t *)rows;
    vm_prof_scope prof(ctx, VM_PROF_APPEND, st);
    const dim3 pgrid((B + 255) / 256, B);
    if (m->dtype == VM_F16) {
        novel_norm_kernel<VM_F16><<<W, 64, 0, st>>>(src, B, D, ws.norm);
        novel_pairs_kernel<VM_F16><<<pgrid, 256, (size_t)D * 2, st>>>(src, B, D, W, ws.norm, threshold, ws.A);
    } else {
        novel_norm_kernel<VM_BF16><<<W, 64, 0, st>>>(src, B, D, ws.norm);
        novel_pairs_kernel<VM_BF16><<<pgrid, 256, (size_t)D * 2, st>>>(src, B, D, W, ws.norm, threshold, ws.A);
    }
    VM_LAUNCH_CHECK(ctx);
    novel_resolve_kernel<<<1, 64, 0, st>>>(ws.A, B, W, threshold, known_scores, known_rows, known_stride, m->d_total,
                                           m->cap, m->ring, ws.hdr, out_count);
    VM_LAUNCH_CHECK(ctx);
    if (m->dtype == VM_F16)
        novel_append_kernel<VM_F16><<<B, 128, 0, st>>>(src, B, D, W, ws.A, ws.hdr, ws.norm, known_rows, known_stride,
                                                      tags, m->rows, m->norm64, m->rnorm32, m->tag, m->cap, m->ring,
                                                      out_keep, out_row_of, m->d_total + VM_GSTATE_OUTSIDE);
    else
        novel_append_kernel<VM_BF16><<<B, 128, 0, st>>>(src, B, D, W, ws.A, ws.hdr, ws.norm, known_rows, known_stride,
                                                       tags, m->rows, m->norm64, m->rnorm32, m->tag, m->cap, m->ring,
                                                       out_keep, out_row_of, m->d_total + VM_GSTATE_OUTSIDE);
    VM_LAUNCH_CHECK(ctx);
    if (m->gkey) {
        novel_group_kernel<<<1, 256, 0, st>>>(keys, B, ws.hdr, m->gkey, m->gord, m->d_total, m->cap, m->ring);
        VM_LAUNCH_CHECK(ctx);
    }
    return VM_OK;
}
