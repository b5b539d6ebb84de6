// Clip search: where does a SEQUENCE of L <= 16 frames occur in the memory (include/vidmem.h vm_topk_cosine_clip,
// DESIGN.md 20)?  The memory holds one row per frame in time order; window r is the rows r .. r+L-1 and scores
// W(r) = mean_i cosine(clip frame i, row r+i), the aligned counterpart of the reference's chunk-to-chunk link
// (src/components/pre_llm_injector.py:346-372).  The k answers are PEAKS: windows that rank before every valid, in-scope
// window closer than min_sep rows (local-maximum suppression, not greedy), so k answers are k moments, not k shifts of one.
//
// Two-stage and certified like the other searches, with which it shares topk_tile_scan.h (the scan; ClipScan is its
// policy), topk_key_image.hip (vm_key_image_select of topk_scope_select.h: cut, compaction, selection over one key per
// slot, 0 = absent), the reference arithmetic of topk_common.h and vm_topk_redo_merge:
//   pack     : each clip -> one zero-padded 16-query tile [C][16][D] + the exact fp64 norm of every frame
//   scan     : fp32 MFMA scores of every live row against the 16 C frames, S[16 c + i][slot] (a tile with no row in a
//              scope of the block's clips costs its tags only and writes nothing: its scores are never read)
//   window   : per (clip, start row) validity and scope from the row count and the L tags, then
//              Bf = (float)((sum_i S_i(slot(r+i)) / ||q_i||) / L), -inf when the window is not valid or not in scope
//   peaks    : key[c][slot(r)] = okey32(Bf(r)) iff no competitor has Bf(r') > Bf(r) + 2 eps_w, else 0.  |Bf - W| <= eps_w
//              = cert_eps(D) + 2^-23 inside the certificate's domain, so a window dropped here has a competitor that
//              exceeds it exactly: provably no peak
//   select   : per clip the best M + 1 possible peaks by (key desc, start asc); > SEL_CAP at the cut -> VM_FLAG_OVERFLOW
//   re-score : one block per (candidate, clip): exact W of the candidate and of every competitor whose Bf is not more than
//              2 eps_w below the candidate's (the others are provably below it), and the exact peak test
//   rank     : per clip the exact peaks among the best M candidates by (W desc, start asc), filtered, k written.  Certified
//              when the clip had at most M possible peaks, or when at least k candidates are exact peaks and the k-th's W
//              is strictly above the (M+1)-th's Bf + eps_w; else VM_FLAG_GAP.  Outside the certificate's norm domain
//              (bf16): VM_FLAG_GAP
//   redo     : flagged clips: exact W of every valid in-scope window into an fp64 array, the exact peak test on that array,
//              a stable top-k of peaks per slice, then vm_topk_redo_merge.  Near-empty when nothing is flagged.
// Every launch reads the row count and the scopes from the device and sizes its grid from the capacity: capturable.
#include "topk_clip_parts.h"
#include "topk_tile_scan.h"

#include <climits>
#include <cmath>

namespace {

constexpr int CLIP_NDMAX = 2 * CLIP_SEPMAX - 1;  // a candidate and its competitors
constexpr int CW_THREADS = 256;    // one thread per start row
constexpr int CR_CHUNK = 1024;     // windows per selection pass of the redo

// |Bf(r) - W(r)| <= eps_w inside the certificate's domain: cert_eps(D) per term and so for their mean,
// below 2^-24 * 1.001 for the one fp32 rounding of |B| <= 1 + eps, below 2^-47 for the fp64 roundings of both sums
__device__ __forceinline__ double clip_eps_w(int D) { return cert_eps(D) + 1.1920928955078125e-07; }

// window o (age order of its start row) is valid and in scope: all L rows live, no tag break inside, every tag in [lo, hi]
__device__ __forceinline__ bool clip_window_ok(const RingView &rv, const int64_t *__restrict__ tag, int64_t o, int L,
                                               int64_t max_gap_ms, bool scoped, int64_t lo, int64_t hi) {
    if (o < 0 || o + L > rv.n) return false;
    if (!tag) return true;
    int64_t tp = tag[slot_of(rv, o)];
    if (scoped && !in_scope(tp, lo, hi)) return false;
    for (int i = 1; i < L; ++i) {
        const int64_t tc = tag[slot_of(rv, o + i)];
        if (clip_tag_break(tp, tc, max_gap_ms)) return false;
        if (scoped && !in_scope(tc, lo, hi)) return false;
        tp = tc;
    }
    return true;
}

// ---- pack --------------------------------------------------------------------------------------------------
// grid (16, C): frame i of clip c -> row 16 c + i of the query tiles (zeros past L) and its exact norm
template <int DT>
__global__ void __launch_bounds__(64)
    clip_pack_kernel(const uint16_t *__restrict__ clips, int L, int D, uint16_t *__restrict__ qt,
                     double *__restrict__ qn) {
    const int i = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    uint4 *dst = reinterpret_cast<uint4 *>(qt + ((size_t)c * CLIP_LMAX + i) * D);
    if (i >= L) {  // uniform
        for (int j = tid; j < D / 8; j += 64) dst[j] = make_uint4(0, 0, 0, 0);
        if (tid == 0) qn[c * CLIP_LMAX + i] = 0.0;
        return;
    }
    const uint16_t *src = clips + ((size_t)c * L + i) * D;
    for (int j = tid; j < D / 8; j += 64) dst[j] = reinterpret_cast<const uint4 *>(src)[j];
    if (tid == 0) qn[c * CLIP_LMAX + i] = __dsqrt_rn(ref_sumsq<DT>(src, D));
}

// ---- scan --------------------------------------------------------------------------------------------------
// The clip policy of the tile scan: the four fp32 scores of a lane go to S[q * fstride + slot], q = 16 clip + frame.
// Scopes (may be null: every row) are per clip; a tile with no row in a scope of the block's clips is not read.
struct ClipScan {
    struct Args {
        const int64_t *tag, *scope_lo, *scope_hi;
        int64_t fstride;
        float *S;
    };
    template <int QT>
    using QState = TagQState<QT>;
    struct View {};
    template <class QS>
    static __device__ __forceinline__ void load_query(QS &qs, const Args &a, int i, int q, bool live) {
        if (a.scope_lo) {
            load_tag_scope(qs, a.scope_lo, a.scope_hi, i, q >> 4, live);  // clips past C have the empty scope
        } else {
            qs.lo[i] = LLONG_MIN;
            qs.hi[i] = LLONG_MAX;
        }
    }
    static __device__ __forceinline__ View view(const Args &, const RingView &) { return {}; }
    template <int QT>
    static __device__ __forceinline__ bool skip_tile(const QState<QT> &qs, const Args &a, const TileLane &l) {
        if (!a.scope_lo) return false;
        return !tile_in_scope<QT>(a.tag, qs.lo, qs.hi, l);  // writes nothing: out-of-scope scores are never read
    }
    template <int QT>
    static __device__ __forceinline__ void epilogue(const QState<QT> &, const Args &a, const View &, const TileLane &l,
                                                    const float (&s)[QT][4]) {
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const int q = l.q0 + 16 * t + l.r16;
            if (q >= l.Q) continue;
            *reinterpret_cast<float4 *>(a.S + (size_t)q * a.fstride + l.p0()) =
                make_float4(s[t][0], s[t][1], s[t][2], s[t][3]);
        }
    }
};

// ---- window ------------------------------------------------------------------------------------------------
// grid (ceil(cap / CW_THREADS), C), thread = start row of age order o: Bf[c][slot(o)] = the fp32 window score, -inf when
// the window is not valid or not in scope
__global__ void __launch_bounds__(CW_THREADS)
    clip_window_kernel(const int64_t *__restrict__ d_total, int64_t cap, int ring, const int64_t *__restrict__ tag,
                       const int64_t *__restrict__ scope_lo, const int64_t *__restrict__ scope_hi, int64_t max_gap_ms,
                       int L, const float *__restrict__ S, int64_t fstride, const double *__restrict__ qn,
                       float *__restrict__ Bf) {
    const int c = blockIdx.y;
    const RingView rv = ring_view(*d_total, cap, ring);
    const int64_t o = (int64_t)blockIdx.x * CW_THREADS + threadIdx.x;
    if (o >= rv.n) return;
    const bool scoped = scope_lo != nullptr;
    const int64_t lo = scoped ? scope_lo[c] : 0, hi = scoped ? scope_hi[c] : 0;
    float bf = -INFINITY;
    if (clip_window_ok(rv, tag, o, L, max_gap_ms, scoped, lo, hi)) {
        double sum = 0.0;
        for (int i = 0; i < L; ++i) {
            const double q = qn[c * CLIP_LMAX + i];
            const float s = S[((size_t)c * CLIP_LMAX + i) * fstride + slot_of(rv, o + i)];
            sum = __dadd_rn(sum, q == 0.0 ? 0.0 : __ddiv_rn((double)s, q));  // a zero frame: an exact 0 on both sides
        }
        bf = (float)__ddiv_rn(sum, (double)L);
    }
    Bf[(size_t)c * fstride + slot_of(rv, o)] = bf;
}

// same grid: key[c][slot(o)] = okey32(Bf) when the window is valid, in scope and a POSSIBLE peak, else 0
__global__ void __launch_bounds__(CW_THREADS)
    clip_peak_kernel(const int64_t *__restrict__ d_total, int64_t cap, int ring, int D, int min_sep,
                     const float *__restrict__ Bf, int64_t fstride, uint32_t *__restrict__ key) {
    const int c = blockIdx.y;
    const RingView rv = ring_view(*d_total, cap, ring);
    const int64_t o = (int64_t)blockIdx.x * CW_THREADS + threadIdx.x;
    if (o >= rv.n) return;
    const float *Bc = Bf + (size_t)c * fstride;
    const int64_t p = slot_of(rv, o);
    const float b = Bc[p];
    uint32_t kv = 0;
    if (b != -INFINITY) {
        const double lim = (double)b + 2.0 * clip_eps_w(D);
        bool possible = true;
        for (int d = 1; d < min_sep; ++d) {
            if (o - d >= 0) {
                const float b2 = Bc[slot_of(rv, o - d)];
                if (b2 != -INFINITY && (double)b2 > lim) possible = false;
            }
            if (o + d < rv.n) {
                const float b2 = Bc[slot_of(rv, o + d)];
                if (b2 != -INFINITY && (double)b2 > lim) possible = false;
            }
        }
        if (possible) kv = okey32(b);
    }
    key[(size_t)c * fstride + p] = kv;
}

// ---- re-score ----------------------------------------------------------------------------------------------
// exact W of window o of clip c from the e_i of its L rows: the sum from 0.0 left to right, one division
template <int DT>
__device__ __forceinline__ double clip_exact_term(const uint16_t *__restrict__ mem, const double *__restrict__ norm64,
                                                  const uint16_t *__restrict__ qt, const double *__restrict__ qn,
                                                  const RingView &rv, int D, int c, int64_t o, int i) {
    const int64_t p = slot_of(rv, o + i);
    const int q = c * CLIP_LMAX + i;
    return ref_cosine(ref_dot<DT>(qt + (size_t)q * D, mem + (size_t)p * D, D), qn[q], norm64[p]);
}

// grid (M + 1, C): block (j, c) = candidate j of clip c.  The exact W of the candidate and of each competitor that could
// rank before it, at most (2 min_sep - 1) L exact dots spread over the block, then the exact peak test.
template <int DT>
__global__ void __launch_bounds__(CW_THREADS)
    clip_rescore_kernel(const uint16_t *__restrict__ mem, const double *__restrict__ norm64,
                        const uint16_t *__restrict__ qt, const double *__restrict__ qn,
                        const int64_t *__restrict__ d_total, int64_t cap, int ring, int D, int L, int min_sep,
                        const float *__restrict__ Bf, int64_t fstride, const int *__restrict__ cand_o,
                        const int *__restrict__ cand_n, double *__restrict__ cand_w, int *__restrict__ cand_p) {
    __shared__ double e[CLIP_NDMAX * CLIP_LMAX];
    __shared__ double wd[CLIP_NDMAX];
    __shared__ int use[CLIP_NDMAX];
    __shared__ int beaten;
    const int j = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    if (j >= cand_n[c]) return;  // uniform; also an overflowed list (-1)
    const RingView rv = ring_view(*d_total, cap, ring);
    const int64_t o = cand_o[(size_t)c * SCMAX + j];
    const float *Bc = Bf + (size_t)c * fstride;
    const int nd = 2 * min_sep - 1, mid = min_sep - 1;
    if (tid < nd) {
        const int64_t o2 = o + tid - mid;
        int u = 0;
        if (o2 >= 0 && o2 < rv.n) {
            const float b2 = Bc[slot_of(rv, o2)];
            // a competitor more than 2 eps_w below the candidate in fp32 is below it exactly
            if (b2 != -INFINITY)
                u = (tid == mid || !((double)b2 < (double)Bc[slot_of(rv, o)] - 2.0 * clip_eps_w(D))) ? 1 : 0;
        }
        use[tid] = u;
    }
    if (tid == 0) beaten = 0;
    __syncthreads();
    for (int t = tid; t < nd * L; t += CW_THREADS) {
        const int w = t / L, i = t - w * L;
        if (use[w]) e[t] = clip_exact_term<DT>(mem, norm64, qt, qn, rv, D, c, o + w - mid, i);
    }
    __syncthreads();
    if (tid < nd && use[tid]) {
        double sum = 0.0;
        for (int i = 0; i < L; ++i) sum = __dadd_rn(sum, e[tid * L + i]);
        wd[tid] = __ddiv_rn(sum, (double)L);
    }
    __syncthreads();
    if (tid < nd && tid != mid && use[tid]) {  // ranks before the candidate: higher W, or the same W and a lower start
        const double w0 = wd[mid], w2 = wd[tid];
        if (w2 > w0 || (w2 == w0 && tid < mid)) beaten = 1;
    }
    __syncthreads();
    if (tid == 0) {
        cand_w[(size_t)c * SCMAX + j] = wd[mid];
        cand_p[(size_t)c * SCMAX + j] = beaten ? 0 : 1;
    }
}

// ---- rank and certify --------------------------------------------------------------------------------------
// One block per clip.  The candidates ranked by (fp32 key desc, start asc): the exact peaks among the first nc = min(C, M)
// are ranked by (W desc, start asc), filtered and written; the (M+1)-th (if any) bounds every other possible peak.
template <int DT>
__global__ void __launch_bounds__(SF_THREADS)
    clip_rank_kernel(const int64_t *__restrict__ d_total, int64_t cap, int ring, int D, int L,
                     const double *__restrict__ qn, const int *__restrict__ cand_o, const uint32_t *__restrict__ cand_k,
                     const int *__restrict__ cand_n, const double *__restrict__ cand_w, const int *__restrict__ cand_p,
                     int M, int k, int use_min, double min_score, int score_mode, double *__restrict__ out_scores,
                     int64_t *__restrict__ out_rows, int *__restrict__ uncertified, int *__restrict__ flags,
                     int *__restrict__ user_flags) {
    __shared__ int so[SCMAX], lo_[SCMAX], sp[SCMAX], lp[SCMAX];
    __shared__ uint32_t sk[SCMAX], lk[SCMAX];
    __shared__ double sw[SCMAX], lw[SCMAX];
    __shared__ int flag_sh;
    const int c = blockIdx.x, tid = threadIdx.x;
    const RingView rv = ring_view(*d_total, cap, ring);
    const int C = cand_n[c];
    if (C < 0) {  // uniform: more possible peaks at the cut than the buffer holds -> the exhaustive redo answers this clip
        for (int i = tid; i < k; i += SF_THREADS) {
            out_scores[(size_t)c * k + i] = 0.0;
            out_rows[(size_t)c * k + i] = -1;
        }
        if (tid == 0) {
            flags[c] = VM_FLAG_OVERFLOW;
            if (user_flags) user_flags[c] = VM_FLAG_OVERFLOW;
            if (uncertified) atomicAdd(uncertified, 1);
        }
        return;
    }
    const int nc = C < M ? C : M;
    if (tid < C) {
        lo_[tid] = cand_o[(size_t)c * SCMAX + tid];
        lk[tid] = cand_k[(size_t)c * SCMAX + tid];
        lw[tid] = cand_w[(size_t)c * SCMAX + tid];
        lp[tid] = cand_p[(size_t)c * SCMAX + tid];
    }
    // with more than M possible peaks the answer stands only once the k-th exact peak clears the (M+1)-th's bound
    if (tid == 0) flag_sh = C > M ? VM_FLAG_GAP : VM_FLAG_CERTIFIED;
    __syncthreads();
    if (tid < C) {  // rank by (fp32 key desc, start asc)
        const int o = lo_[tid];
        const uint32_t key = lk[tid];
        int r = 0;
        for (int j = 0; j < C; ++j) r += (lk[j] > key || (lk[j] == key && lo_[j] < o)) ? 1 : 0;
        so[r] = o;
        sk[r] = key;
        sw[r] = lw[tid];
        sp[r] = lp[tid];
    }
    __syncthreads();
    const bool peak = tid < nc && sp[tid] != 0;
    if (peak) {
        const double w = sw[tid];
        const int o = so[tid];
        int r = 0;
        for (int d = 0; d < nc; ++d) r += (sp[d] && (sw[d] > w || (sw[d] == w && so[d] < o))) ? 1 : 0;
        if (r < k) {
            const double shown = shown_score(w, score_mode);
            const bool pass = passes_min(use_min, shown, min_score);
            out_scores[(size_t)c * k + r] = pass ? shown : 0.0;
            out_rows[(size_t)c * k + r] = pass ? rv.base + o : -1;
        }
        if (r == k - 1 && C > M && w > (double)dekey32(sk[M]) + clip_eps_w(D)) flag_sh = VM_FLAG_CERTIFIED;
    }
    const int npeaks = __syncthreads_count(peak ? 1 : 0);
    for (int i = npeaks + tid; i < k; i += SF_THREADS) {
        out_scores[(size_t)c * k + i] = 0.0;
        out_rows[(size_t)c * k + i] = -1;
    }
    if (tid == 0) {
        int f = flag_sh;
        // domain of the certificate (topk_common.h cert_eps; bf16 only): outside it the in-call redo answers the clip
        if constexpr (DT == VM_BF16) {
            if (f == VM_FLAG_CERTIFIED && rv.n > 0) {
                bool outside = d_total[VM_GSTATE_OUTSIDE] != 0;
                for (int i = 0; i < L; ++i) outside |= cert_norm_outside(qn[c * CLIP_LMAX + i]);
                if (outside) f = VM_FLAG_GAP;
            }
        }
        flags[c] = f;
        if (user_flags) user_flags[c] = f;
        if (f && uncertified) atomicAdd(uncertified, 1);
    }
}

// ---- redo --------------------------------------------------------------------------------------------------
// grid (ceil(cap / CW_THREADS), C): W64[c][o] = the exact W of window o of a flagged clip, -inf when the window is not
// valid or not in scope (indexed by age order)
template <int DT>
__global__ void __launch_bounds__(CW_THREADS)
    clip_redo_score_kernel(const uint16_t *__restrict__ mem, const double *__restrict__ norm64,
                           const uint16_t *__restrict__ qt, const double *__restrict__ qn,
                           const int64_t *__restrict__ d_total, int64_t cap, int ring, int D, int L,
                           const int64_t *__restrict__ tag, const int64_t *__restrict__ scope_lo,
                           const int64_t *__restrict__ scope_hi, int64_t max_gap_ms, const int32_t *__restrict__ flags,
                           int64_t fstride, double *__restrict__ W64) {
    const int c = blockIdx.y;
    if (flags[c] == 0) return;  // uniform
    const RingView rv = ring_view(*d_total, cap, ring);
    const int64_t o = (int64_t)blockIdx.x * CW_THREADS + threadIdx.x;
    if (o >= rv.n) return;
    const bool scoped = scope_lo != nullptr;
    const int64_t lo = scoped ? scope_lo[c] : 0, hi = scoped ? scope_hi[c] : 0;
    double w = -INFINITY;
    if (clip_window_ok(rv, tag, o, L, max_gap_ms, scoped, lo, hi)) {
        double sum = 0.0;
        for (int i = 0; i < L; ++i) sum = __dadd_rn(sum, clip_exact_term<DT>(mem, norm64, qt, qn, rv, D, c, o, i));
        w = __ddiv_rn(sum, (double)L);
    }
    W64[(size_t)c * fstride + o] = w;
}

// grid (nblk, C): block b takes its slice of start rows of a flagged clip, runs the exact peak test on W64 and leaves the
// slice's stable top-k of peaks in part_s / part_o [nblk][C][k] = {W, age order}
__global__ void __launch_bounds__(CW_THREADS)
    clip_redo_slice_kernel(const int64_t *__restrict__ d_total, int64_t cap, int ring, int min_sep, int C, int k,
                           const int32_t *__restrict__ flags, int64_t fstride, const double *__restrict__ W64,
                           double *__restrict__ part_s, int64_t *__restrict__ part_o) {
    __shared__ double sc[CR_CHUNK];
    __shared__ uint8_t live[CR_CHUNK];
    __shared__ double run_s[SKMAX], new_s[SKMAX], red_s[CW_THREADS / 64];
    __shared__ int64_t run_o[SKMAX], new_o[SKMAX], red_o[CW_THREADS / 64];
    const int c = blockIdx.y, tid = threadIdx.x;
    if (flags[c] == 0) return;  // uniform
    const RingView rv = ring_view(*d_total, cap, ring);
    const int64_t per = (rv.n + gridDim.x - 1) / gridDim.x;
    const int64_t lo = (int64_t)blockIdx.x * per;
    const int64_t hi = lo + per < rv.n ? lo + per : rv.n;
    const double *Wc = W64 + (size_t)c * fstride;
    if (tid < k) {
        run_s[tid] = -INFINITY;
        run_o[tid] = -1;
    }
    __syncthreads();
    for (int64_t c0 = lo; c0 < hi; c0 += CR_CHUNK) {
        const int cn = (int)(hi - c0 < CR_CHUNK ? hi - c0 : CR_CHUNK);
        int mine = 0;
        for (int i = tid; i < cn; i += CW_THREADS) {
            const int64_t o = c0 + i;
            const double w = Wc[o];
            bool peak = w != -INFINITY;
            if (peak) {
                for (int d = 1; d < min_sep; ++d) {  // a competitor ranks before: higher W, or the same W at a lower start
                    if (o - d >= 0) {
                        const double w2 = Wc[o - d];
                        if (w2 != -INFINITY && w2 >= w) peak = false;
                    }
                    if (o + d < rv.n) {
                        const double w2 = Wc[o + d];
                        if (w2 != -INFINITY && w2 > w) peak = false;
                    }
                }
            }
            sc[i] = w;
            live[i] = peak ? 1 : 0;
            mine |= peak ? 1 : 0;
        }
        if (!__syncthreads_or(mine)) continue;  // uniform: no peak in this chunk
        block_select<CW_THREADS>(cn + k, k,
                                 [&](int i, double &v, int64_t &o) {
                                     if (i < cn) {
                                         v = sc[i];
                                         o = live[i] ? c0 + i : -1;
                                     } else {
                                         v = run_s[i - cn];
                                         o = run_o[i - cn];
                                     }
                                 },
                                 new_s, new_o, red_s, red_o);
        if (tid < k) {
            run_s[tid] = new_s[tid];
            run_o[tid] = new_o[tid];
        }
        __syncthreads();
    }
    if (tid < k) {
        part_s[((size_t)blockIdx.x * C + c) * k + tid] = run_s[tid];
        part_o[((size_t)blockIdx.x * C + c) * k + tid] = run_o[tid];
    }
}

// ---- host --------------------------------------------------------------------------------------------------
struct CPlan : SelectPlan {  // the select stage's arrays are its base's
    size_t off_qt, off_qn, off_S, off_bf, off_key, off_cw, off_cp, off_flags, off_w64, off_ps, off_po, total;
};

CPlan clip_plan(const vm_memory *m, int C, int k) {
    CPlan p;
    static_cast<TopkGeom &>(p) = vm_topk_geom(m, C * CLIP_LMAX, k, TS_THREADS, VM_REDO_CHUNK_SCOPED);
    p.fstride = (m->cap + 63) / 64 * 64;  // the columns' padding: a tail tile writes its 16 scores
    WsBump ws;
    p.off_qt = ws.take((size_t)C * CLIP_LMAX * m->D * 2);
    p.off_qn = ws.take((size_t)C * CLIP_LMAX * 8);
    p.off_S = ws.take((size_t)C * CLIP_LMAX * (size_t)p.fstride * 4);
    p.off_bf = ws.take((size_t)C * (size_t)p.fstride * 4);
    p.off_key = ws.take((size_t)C * (size_t)p.fstride * 4);
    p.off_co = ws.take((size_t)C * SCMAX * 4);
    p.off_ck = ws.take((size_t)C * SCMAX * 4);
    p.off_cn = ws.take((size_t)C * 4);
    p.off_cw = ws.take((size_t)C * SCMAX * 8);
    p.off_cp = ws.take((size_t)C * SCMAX * 4);
    p.off_flags = ws.take((size_t)C * 4);
    p.off_cut = ws.take((size_t)C * 4);
    p.off_cc = ws.take((size_t)C * 4);
    p.off_cbuf = ws.take((size_t)C * SEL_CAP * 8);
    p.off_w64 = ws.take((size_t)C * (size_t)p.fstride * 8);
    p.off_ps = ws.take((size_t)p.nblk * C * k * 8);
    p.off_po = ws.take((size_t)p.nblk * C * k * 8);
    p.total = ws.off;
    return p;
}

bool clip_shape_ok(int C, int L, int k) { return C >= 1 && L >= 1 && L <= CLIP_LMAX && k >= 1 && k <= SKMAX; }

int clip_check(vm_memory *m, const void *clips, int C, int L, int k, int min_sep, int64_t max_gap_ms,
               const int64_t *scope_lo, const int64_t *scope_hi, int use_min, double min_score, int score_mode,
               const double *out_scores, const int64_t *out_rows, const void *workspace, size_t workspace_bytes,
               const char *who) {
    vm_ctx *ctx = m->ctx;
    if (!clips || !out_scores || !out_rows || C < 1) return vm_fail(ctx, VM_ERR_INVALID, "%s: bad arguments", who);
    if (L < 1 || L > CLIP_LMAX) return vm_fail(ctx, VM_ERR_INVALID, "%s: L=%d outside [1, %d]", who, L, CLIP_LMAX);
    if (k < 1 || k > SKMAX) return vm_fail(ctx, VM_ERR_INVALID, "%s: k=%d outside [1, %d]", who, k, SKMAX);
    if (min_sep < 1 || min_sep > CLIP_SEPMAX)
        return vm_fail(ctx, VM_ERR_INVALID, "%s: min_sep=%d outside [1, %d]", who, min_sep, CLIP_SEPMAX);
    if ((scope_lo == nullptr) != (scope_hi == nullptr))
        return vm_fail(ctx, VM_ERR_INVALID, "%s: one scope array is NULL and the other is not", who);
    if ((scope_lo || max_gap_ms >= 0) && !m->tag)
        return vm_fail(ctx, VM_ERR_INVALID, "%s: scopes and max_gap_ms need a tagged memory (vm_memory_create_tagged)",
                       who);
    if (use_min && std::isnan(min_score)) return vm_fail(ctx, VM_ERR_INVALID, "%s: min_score is NaN", who);
    if (int rc = vm_check_score_mode(ctx, score_mode)) return rc;
    const size_t need = clip_plan(m, C, k).total;
    if (!workspace || workspace_bytes < need)
        return vm_fail(ctx, VM_ERR_NOMEM, "%s: workspace %zu < %zu", who, workspace_bytes, need);
    if (((uintptr_t)workspace & 255) || ((uintptr_t)clips & 15))
        return vm_fail(ctx, VM_ERR_INVALID, "%s: workspace must be 256-byte and clips 16-byte aligned", who);
    return VM_OK;
}

struct ClipCall {
    const void *clips;
    int C, L, k, min_sep;
    int64_t max_gap_ms;
    const int64_t *scope_lo, *scope_hi;
    int use_min;
    double min_score;
    int score_mode;
    double *out_scores;
    int64_t *out_rows;
};

int clip_pack(vm_memory *m, const CPlan &p, const ClipCall &a, char *ws, hipStream_t st) {
    return vm_clip_pack(m, a.clips, a.C, a.L, (uint16_t *)(ws + p.off_qt), (double *)(ws + p.off_qn), st);
}

template <int DT>
int clip_redo(vm_memory *m, const CPlan &p, const ClipCall &a, char *ws, hipStream_t st) {
    vm_ctx *ctx = m->ctx;
    vm_prof_scope prof(ctx, VM_PROF_TOPK_EXACT, st);
    const int32_t *flags = (const int32_t *)(ws + p.off_flags);
    double *W64 = (double *)(ws + p.off_w64);
    double *part_s = (double *)(ws + p.off_ps);
    int64_t *part_o = (int64_t *)(ws + p.off_po);
    const dim3 wgrid((unsigned)((m->cap + CW_THREADS - 1) / CW_THREADS), a.C);
    clip_redo_score_kernel<DT><<<wgrid, CW_THREADS, 0, st>>>(
        m->rows, m->norm64, (const uint16_t *)(ws + p.off_qt), (const double *)(ws + p.off_qn), m->d_total, m->cap,
        m->ring, m->D, a.L, m->tag, a.scope_lo, a.scope_hi, a.max_gap_ms, flags, p.fstride, W64);
    VM_LAUNCH_CHECK(ctx);
    if (int rc = vm_clip_redo_slices(m, p.nblk, a.C, a.k, a.min_sep, flags, p.fstride, W64, part_s, part_o, st)) return rc;
    return vm_topk_redo_merge(m, part_s, part_o, p.nblk, a.C, a.k, flags, a.use_min, a.min_score, a.score_mode, 1, 0,
                              a.out_scores, a.out_rows, nullptr, nullptr, st);
}

template <int DT>
int clip_topk(vm_memory *m, const ClipCall &a, int32_t *out_uncertified, int32_t *out_query_flags, char *ws,
              hipStream_t st) {
    vm_ctx *ctx = m->ctx;
    const CPlan p = clip_plan(m, a.C, a.k);
    const uint16_t *qt = (const uint16_t *)(ws + p.off_qt);
    const double *qn = (const double *)(ws + p.off_qn);
    float *S = (float *)(ws + p.off_S);
    float *Bf = (float *)(ws + p.off_bf);
    uint32_t *key = (uint32_t *)(ws + p.off_key);
    int *cand_o = (int *)(ws + p.off_co);
    uint32_t *cand_k = (uint32_t *)(ws + p.off_ck);
    int *cand_n = (int *)(ws + p.off_cn);
    double *cand_w = (double *)(ws + p.off_cw);
    int *cand_p = (int *)(ws + p.off_cp);
    int *flags = (int *)(ws + p.off_flags);
    {
        vm_prof_scope prof(ctx, VM_PROF_TOPK_SCAN, st);
        if (int rc = clip_pack(m, p, a, ws, st)) return rc;
        if (int rc = vm_clip_scan(m, p, qt, a.C, a.scope_lo, a.scope_hi, p.fstride, S, st)) return rc;
    }
    {
        vm_prof_scope prof(ctx, VM_PROF_TOPK_FINALIZE, st);
        const dim3 wgrid((unsigned)((m->cap + CW_THREADS - 1) / CW_THREADS), a.C);
        clip_window_kernel<<<wgrid, CW_THREADS, 0, st>>>(m->d_total, m->cap, m->ring, m->tag, a.scope_lo, a.scope_hi,
                                                        a.max_gap_ms, a.L, S, p.fstride, qn, Bf);
        VM_LAUNCH_CHECK(ctx);
        if (int rc = vm_clip_peaks(m, a.C, a.min_sep, Bf, p.fstride, key, st)) return rc;
        if (int rc = vm_key_image_select(m, p, key, a.C, ws, st)) return rc;
        clip_rescore_kernel<DT><<<dim3(p.M + 1, a.C), CW_THREADS, 0, st>>>(
            m->rows, m->norm64, qt, qn, m->d_total, m->cap, m->ring, m->D, a.L, a.min_sep, Bf, p.fstride, cand_o, cand_n,
            cand_w, cand_p);
        VM_LAUNCH_CHECK(ctx);
        if (int rc = vm_clip_rank(m, a.C, a.L, qn, cand_o, cand_k, cand_n, cand_w, cand_p, p.M, a.k, a.use_min,
                                  a.min_score, a.score_mode, a.out_scores, a.out_rows, out_uncertified, flags,
                                  out_query_flags, st))
            return rc;
    }
    return clip_redo<DT>(m, p, a, ws, st);
}

template <int DT>
int clip_exact(vm_memory *m, const ClipCall &a, char *ws, hipStream_t st) {
    const CPlan p = clip_plan(m, a.C, a.k);
    if (int rc = clip_pack(m, p, a, ws, st)) return rc;
    if (int rc = vm_fill_flags(m, (int32_t *)(ws + p.off_flags), a.C, st)) return rc;
    return clip_redo<DT>(m, p, a, ws, st);
}

}  // namespace

// ---- the launchers of topk_clip_parts.h ----------------------------------------------------------------------
int vm_clip_pack(vm_memory *m, const void *vectors, int C, int L, uint16_t *qt, double *qn, hipStream_t st) {
    return vm_by_dtype(m, [&](auto dt) -> int {
        clip_pack_kernel<decltype(dt)::value><<<dim3(CLIP_LMAX, C), 64, 0, st>>>((const uint16_t *)vectors, L, m->D, qt, qn);
        VM_LAUNCH_CHECK(m->ctx);
        return VM_OK;
    });
}

int vm_clip_scan(vm_memory *m, const ScanGeom &g, const uint16_t *qt, int C, const int64_t *scope_lo,
                 const int64_t *scope_hi, int64_t fstride, float *S, hipStream_t st) {
    return vm_by_dtype(m, [&](auto dt) -> int {
        return vm_tile_scan<decltype(dt)::value, ClipScan>(m, g, qt, C * CLIP_LMAX,
                                                           {m->tag, scope_lo, scope_hi, fstride, S}, st);
    });
}

int vm_clip_peaks(vm_memory *m, int C, int min_sep, const float *Bf, int64_t fstride, uint32_t *key, hipStream_t st) {
    const dim3 wgrid((unsigned)((m->cap + CW_THREADS - 1) / CW_THREADS), C);
    clip_peak_kernel<<<wgrid, CW_THREADS, 0, st>>>(m->d_total, m->cap, m->ring, m->D, min_sep, Bf, fstride, key);
    VM_LAUNCH_CHECK(m->ctx);
    return VM_OK;
}

int vm_clip_rank(vm_memory *m, int C, int L, const double *qn, const int *cand_o, const uint32_t *cand_k,
                 const int *cand_n, const double *cand_w, const int *cand_p, int M, int k, int use_min, double min_score,
                 int score_mode, double *out_scores, int64_t *out_rows, int32_t *uncertified, int32_t *flags,
                 int32_t *user_flags, hipStream_t st) {
    return vm_by_dtype(m, [&](auto dt) -> int {
        clip_rank_kernel<decltype(dt)::value><<<C, SF_THREADS, 0, st>>>(
            m->d_total, m->cap, m->ring, m->D, L, qn, cand_o, cand_k, cand_n, cand_w, cand_p, M, k, use_min, min_score,
            score_mode, out_scores, out_rows, uncertified, flags, user_flags);
        VM_LAUNCH_CHECK(m->ctx);
        return VM_OK;
    });
}

int vm_clip_redo_slices(vm_memory *m, int nblk, int C, int k, int min_sep, const int32_t *flags, int64_t fstride,
                        const double *W64, double *part_s, int64_t *part_o, hipStream_t st) {
    clip_redo_slice_kernel<<<dim3(nblk, C), CW_THREADS, 0, st>>>(m->d_total, m->cap, m->ring, min_sep, C, k, flags,
                                                                 fstride, W64, part_s, part_o);
    VM_LAUNCH_CHECK(m->ctx);
    return VM_OK;
}

extern "C" size_t vm_topk_clip_workspace_bytes(const vm_memory *m, int C, int L, int k) {
    if (!m || !clip_shape_ok(C, L, k)) return 0;
    return clip_plan(m, C, k).total;
}

extern "C" int vm_topk_cosine_clip(vm_memory *m, const void *clips, int C, int L, int k, int min_sep,
                                   int64_t max_gap_ms, const int64_t *scope_lo, const int64_t *scope_hi,
                                   int use_min_score, double min_score, int score_mode, double *out_scores,
                                   int64_t *out_rows, int32_t *out_uncertified, int32_t *out_query_flags,
                                   void *workspace, size_t workspace_bytes, void *stream) {
    if (!m) return VM_ERR_INVALID;
    const int rc = clip_check(m, clips, C, L, k, min_sep, max_gap_ms, scope_lo, scope_hi, use_min_score, min_score,
                              score_mode, out_scores, out_rows, workspace, workspace_bytes, "vm_topk_cosine_clip");
    if (rc != VM_OK) return rc;
    const ClipCall a = {clips,    C,        L,        k,          min_sep,       max_gap_ms, scope_lo,
                        scope_hi, use_min_score, min_score, score_mode, out_scores, out_rows};
    return vm_by_dtype(m, [&](auto dt) -> int {
        return clip_topk<decltype(dt)::value>(m, a, out_uncertified, out_query_flags, (char *)workspace,
                                              (hipStream_t)stream);
    });
}

extern "C" int vm_topk_cosine_clip_exact(vm_memory *m, const void *clips, int C, int L, int k, int min_sep,
                                         int64_t max_gap_ms, const int64_t *scope_lo, const int64_t *scope_hi,
                                         int use_min_score, double min_score, int score_mode, double *out_scores,
                                         int64_t *out_rows, void *workspace, size_t workspace_bytes, void *stream) {
    if (!m) return VM_ERR_INVALID;
    const int rc = clip_check(m, clips, C, L, k, min_sep, max_gap_ms, scope_lo, scope_hi, use_min_score, min_score,
                              score_mode, out_scores, out_rows, workspace, workspace_bytes, "vm_topk_cosine_clip_exact");
    if (rc != VM_OK) return rc;
    const ClipCall a = {clips,    C,        L,        k,          min_sep,       max_gap_ms, scope_lo,
                        scope_hi, use_min_score, min_score, score_mode, out_scores, out_rows};
    return vm_by_dtype(m, [&](auto dt) -> int {
        return clip_exact<decltype(dt)::value>(m, a, (char *)workspace, (hipStream_t)stream);
    });
}
