// Range search: EVERY stored row whose reference cosine against the query is strictly above a threshold, in ascending
// row id - append order, time order within a video (include/vidmem.h vm_range_cosine).  The call the
// project's other thresholds lacked: HipVectorSearch filters a top-k on min_score
// (src/pipeline/retriever_hybrid.py:296-298), the post-compression filter keeps what scores >= a threshold (:494-504);
// this returns all of it, not the best 64.
//
// The cut is known before the scan starts, so there is no key matrix, no sampling, no selection and no case that cannot
// be certified: a pair whose fp32 score cannot reach the threshold by cert_eps(D) is dropped unscored, every other pair
// is re-scored exactly (topk_common.h), and order comes from prefix sums over separate launches - no atomics, no
// workgroup waits for another.
//   cut      : per query the fp64 norm and one fp32 cut, conservative: a score <= cut is PROVABLY no hit
//   scan     : the shared tile scan (topk_tile_scan.h: 16-row tiles, the row tile the A operand from global memory, the
//              query tile from chunk-swizzled LDS, x 1/||row||; a tile with no in-scope pair is skipped on its 16 tags)
//              with the policy RangeScan below.  One
//              BIT per (query, physical slot): in scope, live, and not at or below the cut.  16 bits per (query, tile),
//              assembled across the four h lanes that hold a tile's rows for one query
//   rescore  : grid (chunks of RC_CHUNK age orders, Q).  Each candidate bit becomes one exact shown score, stored at
//              its age order; the hit bits (age order) and the chunk's hit and candidate counts follow
//   prefix   : per query the exclusive prefix of the chunk hit counts in age order; out_counts, out_rescored
//   emit     : stable compaction of the hit bits: popcount prefixes give every hit its rank, ranks below max_hits
//              write (row id, score); the padding of [count, max_hits) is spread over the same blocks
// The exhaustive entry replaces cut + scan by a mask kernel (every live in-scope pair is a candidate): it shares no
// arithmetic with the scan.  Every launch reads the row count from the device and is sized from the capacity.
#include "topk_tile_scan.h"

#include <climits>
#include <cmath>

namespace {

constexpr int RC_THREADS = 256;  // rescore, emit
constexpr int RC_PER = 16;       // age orders per thread
constexpr int RC_CHUNK = RC_THREADS * RC_PER;  // 4096 age orders = 64 hit words per block
constexpr int RP_THREADS = 256;  // prefix (one block per query)

// the hit rule on an exact cosine: shown score strictly above the threshold
__device__ __forceinline__ bool is_hit(double shown, double min_score) { return passes_min(1, shown, min_score); }

// ---- cut ---------------------------------------------------------------------------------------------------
// One thread per query.  qn[q] = the reference norm.  cut[q]: every fp32 scan score s <= cut[q] is provably no hit: the
// exact cosine is at most (double)s / ||q|| + cert_eps(D) - the expression clears_gap uses for a rejected row - and
// shown_score is monotone, so is_hit of that bound being false settles it.  The candidate value (threshold - eps) x ||q||
// is rounded DOWN to fp32 and then verified with the very predicate, stepping further down while it fails: a row just
// below the cut is still a candidate, never the reverse.  A zero query scores 0.0 everywhere: all or nothing.
// The bound holds inside the certificate's domain only (topk_common.h cert_eps).  A bf16 query whose norm lies outside
// it, or a bf16 memory whose domain word is set (dom = &d_total[VM_GSTATE_OUTSIDE]: some stored row's norm does), gets
// the cut NaN: every in-scope pair is a candidate and is settled exactly.  fp16 norms cannot leave the domain.
template <int DT>
__global__ void __launch_bounds__(64)
    range_cut_kernel(const uint16_t *__restrict__ queries, int Q, int D, double min_score, int score_mode,
                     float *__restrict__ cut, double *__restrict__ qn_out, const int64_t *dom) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= Q) return;
    const double qn = __dsqrt_rn(ref_sumsq<DT>(queries + (size_t)q * D, D));
    qn_out[q] = qn;
    bool off_domain = false;
    if constexpr (DT == VM_BF16) off_domain = *dom != 0 || cert_norm_outside(qn);
    float c;
    if (qn == 0.0) {
        c = is_hit(shown_score(0.0, score_mode), min_score) ? -INFINITY : INFINITY;
    } else if (off_domain) {
        c = NAN;  // no fp32 score is `at or below` a NaN cut - not even -inf, which an overflowed sum is: all candidates
    } else {
        const double eps = cert_eps(D);
        auto rejects = [&](float s) { return !is_hit(shown_score((double)s / qn + eps, score_mode), min_score); };
        const double raw = score_mode == VM_SCORE_UNIT_INTERVAL ? 2.0 * min_score - 1.0 : min_score;
        c = __double2float_rd((raw - eps) * qn);
        for (int it = 0; it < 4 && !rejects(c); ++it) c = nextafterf(c, -INFINITY);
        if (!rejects(c)) c = -INFINITY;  // not reached for finite operands; every row is then a candidate
    }
    cut[q] = c;
}

// ---- scan --------------------------------------------------------------------------------------------------
// The range policy of the tile scan (topk_tile_scan.h): lane (r16, h) holds 4 of a tile's 16 pair bits for its query, the
// other 12 sit in lanes r16 + 16 h'.  cand16[q * cstride16 + tile] = the tile's 16 bits (bit i = slot tile*16 + i).
// SCOPED = false reads no tags (every live row is in scope) and skips no tile.
template <int QT, bool SCOPED>
struct RangeQState : TagQState<QT> {  // the scopes (topk_tile_scan.h), then the cuts
    float cut[QT * 16];
};
template <int QT>
struct RangeQState<QT, false> {
    float cut[QT * 16];
};
template <bool SCOPED>
struct RangeScan {
    struct Args {
        const int64_t *tag, *scope_lo, *scope_hi;
        const float *cut;
        int64_t cstride16;
        uint16_t *cand16;
    };
    template <int QT>
    using QState = RangeQState<QT, SCOPED>;
    struct View {};
    template <class QS>
    static __device__ __forceinline__ void load_query(QS &qs, const Args &a, int i, int q, bool live) {
        // queries past Q have the empty scope and are never written
        if constexpr (SCOPED) load_tag_scope(qs, a.scope_lo, a.scope_hi, i, q, live);
        qs.cut[i] = live ? a.cut[q] : INFINITY;
    }
    static __device__ __forceinline__ View view(const Args &, const RingView &) { return {}; }
    template <int QT>
    static __device__ __forceinline__ bool skip_tile(const QState<QT> &qs, const Args &a, const TileLane &l) {
        if constexpr (SCOPED) {
            if (tile_in_scope<QT>(a.tag, qs.lo, qs.hi, l)) return false;
#pragma unroll
            for (int t = 0; t < QT; ++t) {  // a skipped tile has no candidate
                const int q = l.q0 + 16 * t + l.r16;
                if (l.h == 0 && q < l.Q) a.cand16[(size_t)q * a.cstride16 + l.tile] = 0;
            }
            return true;
        } else {
            return false;
        }
    }
    template <int QT>
    static __device__ __forceinline__ void epilogue(const QState<QT> &qs, const Args &a, const View &,
                                                    const TileLane &l, const float (&s)[QT][4]) {
        int64_t tj[4] = {0, 0, 0, 0};
        if constexpr (SCOPED) {
#pragma unroll
            for (int j = 0; j < 4; ++j) tj[j] = a.tag[l.p0() + j];
        }
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const int q = l.q0 + 16 * t + l.r16;  // past Q: cut = +inf and an empty scope, no bit; all 64 lanes shuffle
            const float c = qs.cut[16 * t + l.r16];
            int64_t lo = 0, hi = 0;
            if constexpr (SCOPED) {
                lo = qs.lo[16 * t + l.r16];
                hi = qs.hi[16 * t + l.r16];
            }
            uint32_t bits = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = l.p0() + j < l.n && (!SCOPED || in_scope(tj[j], lo, hi));
                // `not at or below the cut`: a NaN score stays a candidate and is settled exactly
                if (in && !(s[t][j] <= c)) bits |= 1u << (4 * l.h + j);
            }
            bits |= __shfl_xor(bits, 16, 64);
            bits |= __shfl_xor(bits, 32, 64);
            if (l.h == 0 && q < l.Q) a.cand16[(size_t)q * a.cstride16 + l.tile] = (uint16_t)bits;
        }
    }
};

// ---- mask (exhaustive entry) -------------------------------------------------------------------------------
// grid (words, Q): candidate word w of query q = the live, in-scope slots among [32 w, 32 w + 32).  No score is looked at.
__global__ void __launch_bounds__(256)
    range_mask_kernel(const int64_t *__restrict__ tag, const int64_t *__restrict__ scope_lo,
                      const int64_t *__restrict__ scope_hi, const int64_t *__restrict__ d_total, int64_t cap, int ring,
                      int64_t cstride32, uint32_t *__restrict__ cand32) {
    const int q = blockIdx.y;
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= cstride32) return;
    const int64_t n = ring_view(*d_total, cap, ring).n;
    uint32_t bits = 0;
    if (w * 32 < n) {
        const bool scoped = scope_lo != nullptr;
        const int64_t lo = scoped ? scope_lo[q] : 0, hi = scoped ? scope_hi[q] : 0;
        for (int b = 0; b < 32; ++b) {
            const int64_t p = w * 32 + b;
            if (p < n && (!scoped || in_scope(tag[p], lo, hi))) bits |= 1u << b;
        }
    }
    cand32[(size_t)q * cstride32 + w] = bits;
}

// ---- rescore -----------------------------------------------------------------------------------------------
// grid (chunks, Q).  Thread tid owns the age orders o0 + i * RC_THREADS + tid, so that one wave's ballot is one 64-bit
// word of hit bits.  A chunk without a candidate leaves before it loads the query.
template <int DT>
__global__ void __launch_bounds__(RC_THREADS)
    range_rescore_kernel(const uint16_t *__restrict__ mem, const double *__restrict__ norm64,
                         const uint16_t *__restrict__ queries, const double *__restrict__ qn_arr,
                         const int64_t *__restrict__ d_total, int64_t cap, int ring, int D,
                         const uint32_t *__restrict__ cand32, int64_t cstride32, double min_score, int score_mode,
                         double *__restrict__ scores, int64_t sstride, unsigned long long *__restrict__ hit64,
                         int64_t hstride, int *__restrict__ chunk_hits, int *__restrict__ chunk_cands, int nch) {
    extern __shared__ __attribute__((aligned(16))) char rc_dyn[];
    uint16_t *ql = reinterpret_cast<uint16_t *>(rc_dyn);  // [D]
    __shared__ int red[2][RC_THREADS / 64];
    const int q = blockIdx.y, c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RingView rv = ring_view(*d_total, cap, ring);
    const int64_t o0 = (int64_t)c * RC_CHUNK;
    const uint32_t *cq = cand32 + (size_t)q * cstride32;
    uint32_t mine = 0;  // bit i: age order o0 + i * RC_THREADS + tid is a candidate
    for (int i = 0; i < RC_PER; ++i) {
        const int64_t o = o0 + (int64_t)i * RC_THREADS + tid;
        if (o < rv.n) {
            const int64_t p = slot_of(rv, o);
            mine |= ((cq[p >> 5] >> (p & 31)) & 1u) << i;
        }
    }
    unsigned long long *hq = hit64 + (size_t)q * hstride + (size_t)c * (RC_CHUNK / 64);
    const int64_t hwords = hstride - (int64_t)c * (RC_CHUNK / 64);  // words of this chunk inside the column
    if (!__syncthreads_or(mine != 0)) {  // uniform
        if (o0 < rv.n && tid < RC_CHUNK / 64 && tid < hwords) hq[tid] = 0ull;
        if (tid == 0) {
            chunk_hits[(size_t)q * nch + c] = 0;
            chunk_cands[(size_t)q * nch + c] = 0;
        }
        return;
    }
    for (int i = tid; i < D / 8; i += RC_THREADS)
        reinterpret_cast<uint4 *>(ql)[i] = reinterpret_cast<const uint4 *>(queries + (size_t)q * D)[i];
    __syncthreads();
    const double qn = qn_arr[q];
    int nh = 0, nc = 0;
    for (int i = 0; i < RC_PER; ++i) {
        bool hit = false;
        if ((mine >> i) & 1u) {
            const int64_t o = o0 + (int64_t)i * RC_THREADS + tid;
            const int64_t p = slot_of(rv, o);
            const double shown =
                shown_score(ref_cosine(ref_dot<DT>(ql, mem + (size_t)p * D, D), qn, norm64[p]), score_mode);
            scores[(size_t)q * sstride + o] = shown;
            hit = is_hit(shown, min_score);
            ++nc;
        }
        const unsigned long long word = __ballot(hit);
        const int wi = i * (RC_THREADS / 64) + wave;
        if (lane == 0 && wi < hwords) hq[wi] = word;
        nh += hit ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        nh += __shfl_xor(nh, off, 64);
        nc += __shfl_xor(nc, off, 64);
    }
    if (lane == 0) {
        red[0][wave] = nh;
        red[1][wave] = nc;
    }
    __syncthreads();
    if (tid == 0) {
        int th = 0, tc = 0;
#pragma unroll
        for (int w = 0; w < RC_THREADS / 64; ++w) {
            th += red[0][w];
            tc += red[1][w];
        }
        chunk_hits[(size_t)q * nch + c] = th;
        chunk_cands[(size_t)q * nch + c] = tc;
    }
}

// ---- prefix ------------------------------------------------------------------------------------------------
// One block per query: chunk_base[c] = hits in the chunks before c (age order: in a wrapped ring the chunks already
// start at the head); the totals go to out_counts / out_rescored.
__global__ void __launch_bounds__(RP_THREADS)
    range_prefix_kernel(const int *__restrict__ chunk_hits, const int *__restrict__ chunk_cands, int nch,
                        int64_t *__restrict__ chunk_base, int64_t *__restrict__ out_counts,
                        int64_t *__restrict__ out_rescored) {
    __shared__ int64_t wsum[2][RP_THREADS / 64];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (nch + RP_THREADS - 1) / RP_THREADS;
    const int c0 = tid * per, c1 = c0 + per < nch ? c0 + per : nch;
    const int *ch = chunk_hits + (size_t)q * nch, *cc = chunk_cands + (size_t)q * nch;
    int64_t hs = 0, cs = 0;
    for (int c = c0; c < c1; ++c) {
        hs += ch[c];
        cs += cc[c];
    }
    int64_t inc = hs;  // inclusive scan of the threads' hit sums
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t v = __shfl_up(inc, off, 64);
        if (lane >= off) inc += v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cs += __shfl_xor(cs, off, 64);
    if (lane == 63) wsum[0][wave] = inc;
    if (lane == 0) wsum[1][wave] = cs;
    __syncthreads();
    int64_t before = 0, total = 0, cands = 0;
#pragma unroll
    for (int w = 0; w < RP_THREADS / 64; ++w) {
        if (w < wave) before += wsum[0][w];
        total += wsum[0][w];
        cands += wsum[1][w];
    }
    int64_t run = before + inc - hs;
    for (int c = c0; c < c1; ++c) {
        chunk_base[(size_t)q * nch + c] = run;
        run += ch[c];
    }
    if (tid == 0) {
        out_counts[q] = total;
        if (out_rescored) out_rescored[q] = cands;
    }
}

// ---- emit --------------------------------------------------------------------------------------------------
// grid (chunks, Q).  rank of a hit = chunk_base + hits in the chunk's earlier words + hits below it in its word.
__global__ void __launch_bounds__(RC_THREADS)
    range_emit_kernel(const int64_t *__restrict__ d_total, int64_t cap, int ring,
                      const unsigned long long *__restrict__ hit64, int64_t hstride, const double *__restrict__ scores,
                      int64_t sstride, const int *__restrict__ chunk_hits, const int64_t *__restrict__ chunk_base,
                      int nch, const int64_t *__restrict__ counts, int64_t max_hits, int64_t row_stride,
                      int64_t row_offset, int64_t *__restrict__ out_rows, double *__restrict__ out_scores) {
    __shared__ unsigned long long words[RC_CHUNK / 64];
    __shared__ int wbase[RC_CHUNK / 64];
    const int q = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
    int64_t *orow = out_rows + (size_t)q * max_hits;
    double *osc = out_scores + (size_t)q * max_hits;
    for (int64_t i = counts[q] + (int64_t)c * RC_THREADS + tid; i < max_hits; i += (int64_t)gridDim.x * RC_THREADS) {
        orow[i] = -1;
        osc[i] = 0.0;
    }
    const int nh = chunk_hits[(size_t)q * nch + c];
    const int64_t base = chunk_base[(size_t)q * nch + c];
    if (nh == 0 || base >= max_hits) return;  // uniform
    const RingView rv = ring_view(*d_total, cap, ring);
    if (tid < RC_CHUNK / 64) {  // one wave: the exclusive prefix of the words' popcounts
        const int64_t wi = (int64_t)c * (RC_CHUNK / 64) + tid;
        const unsigned long long w = wi < hstride ? hit64[(size_t)q * hstride + wi] : 0ull;
        const int pc = __popcll(w);
        int inc = pc;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(inc, off, 64);
            if (tid >= off) inc += v;
        }
        words[tid] = w;
        wbase[tid] = inc - pc;
    }
    __syncthreads();
    const int64_t o0 = (int64_t)c * RC_CHUNK;
    for (int i = 0; i < RC_PER; ++i) {
        const int ol = i * RC_THREADS + tid;
        const unsigned long long w = words[ol >> 6];
        const int b = ol & 63;
        if ((w >> b) & 1ull) {
            const int64_t rank = base + wbase[ol >> 6] + __popcll(w & ((1ull << b) - 1ull));
            if (rank < max_hits) {
                orow[rank] = (rv.base + o0 + ol) * row_stride + row_offset;
                osc[rank] = scores[(size_t)q * sstride + o0 + ol];
            }
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------
struct RPlan : ScanGeom {
    int64_t cap_pad;  // the columns' padding (64 rows)
    int nch;          // chunks of RC_CHUNK age orders
    size_t off_hit, off_sc, off_ch, off_cc, off_cb, off_cut, off_qn, total;
};

RPlan range_plan(const vm_memory *m, int Q) {
    RPlan p;
    p.cap_pad = (m->cap + 63) / 64 * 64;
    p.nch = (int)((p.cap_pad + RC_CHUNK - 1) / RC_CHUNK);
    static_cast<ScanGeom &>(p) = vm_scan_geom(m, Q, p.cap_pad / 16, TS_THREADS);  // the tiles of the padded columns
    WsBump ws;
    ws.take((size_t)Q * (size_t)p.cap_pad / 8);              // candidate bits at offset 0: [Q][physical slot]
    p.off_hit = ws.take((size_t)Q * (size_t)p.cap_pad / 8);  // hit bits [Q][age order]
    p.off_sc = ws.take((size_t)Q * (size_t)p.cap_pad * 8);   // exact shown scores [Q][age order], candidates only
    p.off_ch = ws.take((size_t)Q * p.nch * 4);
    p.off_cc = ws.take((size_t)Q * p.nch * 4);
    p.off_cb = ws.take((size_t)Q * p.nch * 8);
    p.off_cut = ws.take((size_t)Q * 4);
    p.off_qn = ws.take((size_t)Q * 8);
    p.total = ws.off;
    return p;
}

int range_check(vm_memory *m, const void *queries, int Q, double min_score, int score_mode, const int64_t *scope_lo,
                const int64_t *scope_hi, int64_t max_hits, const int64_t *out_rows, const double *out_scores,
                const int64_t *out_counts, const void *workspace, size_t workspace_bytes, const char *who) {
    vm_ctx *ctx = m->ctx;
    if (!queries || Q <= 0 || max_hits < 0 || !out_counts || (max_hits > 0 && (!out_rows || !out_scores)))
        return vm_fail(ctx, VM_ERR_INVALID, "%s: bad arguments", who);
    if ((scope_lo == nullptr) != (scope_hi == nullptr))
        return vm_fail(ctx, VM_ERR_INVALID, "%s: scope_lo and scope_hi are given together or not at all", who);
    if (scope_lo && !m->tag)
        return vm_fail(ctx, VM_ERR_INVALID, "%s: the memory is not tagged (vm_memory_create_tagged)", who);
    if (std::isnan(min_score)) return vm_fail(ctx, VM_ERR_INVALID, "%s: min_score is NaN", who);
    if (int rc = vm_check_score_mode(ctx, score_mode)) return rc;
    const size_t need = range_plan(m, Q).total;
    if (!workspace || workspace_bytes < need)
        return vm_fail(ctx, VM_ERR_NOMEM, "%s: workspace %zu < %zu", who, workspace_bytes, need);
    if (((uintptr_t)workspace & 255) || ((uintptr_t)queries & 15))
        return vm_fail(ctx, VM_ERR_INVALID, "%s: workspace must be 256-byte and queries 16-byte aligned", who);
    return VM_OK;
}

// fast = cut + scan, otherwise the mask; then rescore, prefix, emit
template <int DT>
int range_run(vm_memory *m, bool fast, const void *queries, int Q, double min_score, int score_mode,
              const int64_t *scope_lo, const int64_t *scope_hi, int64_t row_stride, int64_t row_offset,
              int64_t max_hits, int64_t *out_rows, double *out_scores, int64_t *out_counts, int64_t *out_rescored,
              char *ws, hipStream_t st) {
    vm_ctx *ctx = m->ctx;
    const RPlan p = range_plan(m, Q);
    uint32_t *cand32 = (uint32_t *)ws;
    unsigned long long *hit64 = (unsigned long long *)(ws + p.off_hit);
    double *scores = (double *)(ws + p.off_sc);
    int *chunk_hits = (int *)(ws + p.off_ch), *chunk_cands = (int *)(ws + p.off_cc);
    int64_t *chunk_base = (int64_t *)(ws + p.off_cb);
    float *cut = (float *)(ws + p.off_cut);
    double *qn = (double *)(ws + p.off_qn);
    const int64_t cstride32 = p.cap_pad / 32;
    {
        vm_prof_scope prof(ctx, fast ? VM_PROF_TOPK_SCAN : VM_PROF_TOPK_EXACT, st);
        range_cut_kernel<DT><<<(Q + 63) / 64, 64, 0, st>>>((const uint16_t *)queries, Q, m->D, min_score, score_mode,
                                                          cut, qn, m->d_total + VM_GSTATE_OUTSIDE);
        VM_LAUNCH_CHECK(ctx);
        if (fast) {
            const int64_t cstride16 = p.cap_pad / 16;
            uint16_t *c16 = (uint16_t *)ws;
            const int rc = scope_lo ? vm_tile_scan<DT, RangeScan<true>>(
                                          m, p, queries, Q, {m->tag, scope_lo, scope_hi, cut, cstride16, c16}, st)
                                    : vm_tile_scan<DT, RangeScan<false>>(
                                          m, p, queries, Q, {nullptr, nullptr, nullptr, cut, cstride16, c16}, st);
            if (rc != VM_OK) return rc;
        } else {
            range_mask_kernel<<<dim3((unsigned)((cstride32 + 255) / 256), Q), 256, 0, st>>>(
                m->tag, scope_lo, scope_hi, m->d_total, m->cap, m->ring, cstride32, cand32);
            VM_LAUNCH_CHECK(ctx);
        }
    }
    vm_prof_scope prof(ctx, fast ? VM_PROF_TOPK_FINALIZE : VM_PROF_TOPK_EXACT, st);
    range_rescore_kernel<DT><<<dim3(p.nch, Q), RC_THREADS, (size_t)m->D * 2, st>>>(
        m->rows, m->norm64, (const uint16_t *)queries, qn, m->d_total, m->cap, m->ring, m->D, cand32, cstride32,
        min_score, score_mode, scores, p.cap_pad, hit64, p.cap_pad / 64, chunk_hits, chunk_cands, p.nch);
    VM_LAUNCH_CHECK(ctx);
    range_prefix_kernel<<<Q, RP_THREADS, 0, st>>>(chunk_hits, chunk_cands, p.nch, chunk_base, out_counts, out_rescored);
    VM_LAUNCH_CHECK(ctx);
    if (max_hits > 0) {
        range_emit_kernel<<<dim3(p.nch, Q), RC_THREADS, 0, st>>>(m->d_total, m->cap, m->ring, hit64, p.cap_pad / 64,
                                                                 scores, p.cap_pad, chunk_hits, chunk_base, p.nch,
                                                                 out_counts, max_hits, row_stride, row_offset, out_rows,
                                                                 out_scores);
        VM_LAUNCH_CHECK(ctx);
    }
    return VM_OK;
}

int range_entry(vm_memory *m, bool fast, const void *queries, int Q, double min_score, int score_mode,
                const int64_t *scope_lo, const int64_t *scope_hi, int64_t row_stride, int64_t row_offset,
                int64_t max_hits, int64_t *out_rows, double *out_scores, int64_t *out_counts, int64_t *out_rescored,
                void *workspace, size_t workspace_bytes, void *stream, const char *who) {
    if (!m) return VM_ERR_INVALID;
    const int rc = range_check(m, queries, Q, min_score, score_mode, scope_lo, scope_hi, max_hits, out_rows, out_scores,
                               out_counts, workspace, workspace_bytes, who);
    if (rc != VM_OK) return rc;
    return vm_by_dtype(m, [&](auto dt) {
        return range_run<decltype(dt)::value>(m, fast, queries, Q, min_score, score_mode, scope_lo, scope_hi,
                                              row_stride, row_offset, max_hits, out_rows, out_scores, out_counts,
                                              out_rescored, (char *)workspace, (hipStream_t)stream);
    });
}

}  // namespace

extern "C" size_t vm_range_workspace_bytes(const vm_memory *m, int Q) {
    if (!m || Q <= 0) return 0;
    return range_plan(m, Q).total;
}

extern "C" int vm_range_cosine(vm_memory *m, const void *queries, int Q, double min_score, int score_mode,
                               const int64_t *scope_lo, const int64_t *scope_hi, int64_t row_stride, int64_t row_offset,
                               int64_t max_hits, int64_t *out_rows, double *out_scores, int64_t *out_counts,
                               int64_t *out_rescored, void *workspace, size_t workspace_bytes, void *stream) {
    return range_entry(m, true, queries, Q, min_score, score_mode, scope_lo, scope_hi, row_stride, row_offset, max_hits,
                       out_rows, out_scores, out_counts, out_rescored, workspace, workspace_bytes, stream,
                       "vm_range_cosine");
}

extern "C" int vm_range_cosine_exact(vm_memory *m, const void *queries, int Q, double min_score, int score_mode,
                                     const int64_t *scope_lo, const int64_t *scope_hi, int64_t row_stride,
                                     int64_t row_offset, int64_t max_hits, int64_t *out_rows, double *out_scores,
                                     int64_t *out_counts, void *workspace, size_t workspace_bytes, void *stream) {
    return range_entry(m, false, queries, Q, min_score, score_mode, scope_lo, scope_hi, row_stride, row_offset,
                       max_hits, out_rows, out_scores, out_counts, nullptr, workspace, workspace_bytes, stream,
                       "vm_range_cosine_exact");
}
