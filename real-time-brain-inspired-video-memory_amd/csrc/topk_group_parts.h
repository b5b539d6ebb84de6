// What the grouped search (topk_group.hip) and the scoped grouped search (topk_group_scope.hip) share beyond
// topk_select.h, all of it from topk_group.hip:
//   moved unchanged   the tuning constants, the fp64 key images, the exact re-score, radix_select_all, the workspace
//                     plan; group_table_kernel and group_compact_kernel, which are no templates: compiled once, in
//                     topk_group_parts.hip, and reached through the two launchers declared below
//   moved and changed group_fold_runs (GroupScan's epilogue, its key now a functor), group_finalize_kernel and
//                     group_redo_scan_kernel (a row predicate SC of vm_internal.h passed by value, used under
//                     `if constexpr (SC::scoped)` only; the redo's LDS score array is `rs`, since `sc` is the predicate)
//   the host driver   GroupCall, grouped_topk, grouped_redo, grouped_exact: a search brings its scan policy, its two
//                     select kernels and its predicate
// What stays in the anonymous namespace here is a template, or inlined into one: each is instantiated in one unit only.
// topk_scope_select.h reuses constant names with other values (SEL_CAP): no unit may include both headers.
#pragma once
#include "topk_tile_scan.h"

#include <climits>

// ---- table and compaction (topk_group_parts.hip) ------------------------------------------------------------------
// first_o[g] = age order of the first live row of live group g, first_o[ng] = n; F (if not null): F[0, Q * ng) = 0;
// fill_flags: flags[0, Q) = 1 (the exhaustive-only entry point)
int vm_group_table(vm_memory *m, int blocks, int Q, int *first_o, uint32_t *F, int32_t *flags, int fill_flags,
                   hipStream_t st);
// grid (slices, Q): every group whose composite is >= cut[q] goes to the query's buffer; ccount[q] > SEL_CAP: radix path
int vm_group_compact(vm_memory *m, int slices, int Q, const uint32_t *F, const unsigned long long *cut, int *ccount,
                     unsigned long long *cbuf, hipStream_t st);

namespace {

constexpr int SEL_THREADS = 1024; // select: cut and final sort (one block per query)
constexpr int SEL_SAMPLE = 2048;  // groups whose fp32 maxima give each query's cut
constexpr int SEL_CAP = 4096;     // groups at or above the cut a query keeps; more -> the full radix select
constexpr int CMP_THREADS = 256;  // select: compaction
constexpr int CMP_LCAP = 1024;    // hits one compaction block gathers in LDS
constexpr int GF_THREADS = 512;   // finalize
constexpr int GCMAX = 128;        // candidate groups per query kept by the select (M + 1 <= GCMAX)
constexpr int GROWCAP = 4096;     // rows the finalize re-scores per query; more -> VM_FLAG_OVERFLOW, exhaustive redo
constexpr int GR_THREADS = 256;   // redo
constexpr int GR_CHUNK = 1024;    // rows scored per selection pass of the redo
constexpr int GKMAX = 64;

// order-preserving unsigned images of fp64 scores (okey32 / dekey32 of topk_select.h, one word wider)
__device__ __forceinline__ unsigned long long okey64(double d) {
    unsigned long long u = (unsigned long long)__double_as_longlong(d);
    if (d == 0.0) u = 0;
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double dekey64(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// the exact reference cosine of the query staged in LDS (ql) and the row in slot p, strictly left to right.  The loops
// here are topk_common.h's ref_dot and ref_sumsq written out: called as helpers they change the finalize's instructions.
template <int DT>
__device__ __forceinline__ double exact_score(const uint16_t *ql, double qn, const uint16_t *__restrict__ mem,
                                              const double *__restrict__ norm64, int64_t p, int D) {
    using E = vm_elem<DT>;
    const uint16_t *mv = mem + (size_t)p * D;
    double dot = 0.0;
    for (int i = 0; i < D; i += 32) {  // D is a multiple of 128; 4 row chunks in flight per step
        uint4 b4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) b4[u] = *reinterpret_cast<const uint4 *>(mv + i + 8 * u);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint4 a = *reinterpret_cast<const uint4 *>(ql + i + 8 * u);
            const uint16_t *ae = reinterpret_cast<const uint16_t *>(&a);
            const uint16_t *be = reinterpret_cast<const uint16_t *>(&b4[u]);
#pragma unroll
            for (int j = 0; j < 8; ++j) dot = __dadd_rn(dot, __dmul_rn(E::to_double(ae[j]), E::to_double(be[j])));
        }
    }
    const double mn = norm64[p];  // the reference's norm of the stored row, computed at append
    return ref_cosine(dot, qn, mn);
}

template <int DT>
__device__ __forceinline__ double exact_qnorm(const uint16_t *ql, int D) {
    using E = vm_elem<DT>;
    double nq = 0.0;
    for (int i = 0; i < D; i += 8) {  // 16-byte LDS reads; the sum itself strictly left to right
        const uint4 a = *reinterpret_cast<const uint4 *>(ql + i);
        const uint16_t *ae = reinterpret_cast<const uint16_t *>(&a);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double x = E::to_double(ae[j]);
            nq = __dadd_rn(nq, __dmul_rn(x, x));
        }
    }
    return __dsqrt_rn(nq);
}


// ---- scan: run folding ------------------------------------------------------------------------------------------
// The epilogue of the grouped tile-scan policies.  Instead of a key per row, each lane folds its 4 consecutive rows into
// runs of one group and raises F[q * ng + group] with one atomic max per run.  key_of(t, j, score): the key of the
// lane's row j for query tile t - okey32(score), or 0 for a (query, row) pair that does not count (an atomic max with 0
// is a no-op on the cleared maxima, so the run structure, which is per row, needs no case for it).
template <int QT, class KeyOf>
__device__ __forceinline__ void group_fold_runs(const int64_t *gord, uint32_t *F,
                                                const GroupView &gv, const TileLane &l, const float (&s)[QT][4],
                                                KeyOf key_of) {
    const int lane = l.lane, h = l.h;
    int gj[4];  // live group index (< cap < 2^31), -1 past the live rows
#pragma unroll
    for (int j = 0; j < 4; ++j) gj[j] = l.p0() + j < l.n ? (int)(gord[l.p0() + j] - gv.ord0) : -1;
    // physical slot p holds age order p - head (mod cap); the ordinal does not care: groups are runs of slots too,
    // except across the physical wrap, where the two halves still carry one ordinal
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int q = l.q0 + 16 * t + l.r16, Q = l.Q;
        uint32_t *Fq = F + (size_t)q * gv.ng;
        // Runs of one group among this lane's 4 rows.  Interior runs go straight to their atomic.  The first and
        // the last run may go on in the lanes that hold the rows before / after (lane -+ 16, same query), so one
        // atomic per run of the whole 16-row tile: the lane where the run starts adds what the next lanes hold.
        int gF = -1, gL = -1, closed = 0;
        uint32_t bF = 0, bL = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (gj[j] < 0) continue;
            const uint32_t key = key_of(t, j, s[t][j]);
            if (gj[j] != gL) {
                if (gL >= 0) {  // the run before closes
                    if (closed == 0) {
                        gF = gL;
                        bF = bL;
                    } else if (q < Q) {
                        atomicMax(Fq + gL, bL);
                    }
                    ++closed;
                }
                gL = gj[j];
                bL = key;
            } else {
                bL = key > bL ? key : bL;
            }
        }
        const int single = closed == 0;  // one run (or none): it is the first and the last
        if (single) {
            gF = gL;
            bF = bL;
        }
        // neighbours, fetched by every lane (the four lanes of a query are all live or all idle together)
        const int gLp = __shfl(gL, (lane - 16) & 63, 64);
        int gFn[3], sn[3];
        uint32_t bFn[3];
#pragma unroll
        for (int d = 1; d <= 3; ++d) {
            gFn[d - 1] = __shfl(gF, (lane + 16 * d) & 63, 64);
            bFn[d - 1] = __shfl(bF, (lane + 16 * d) & 63, 64);
            sn[d - 1] = __shfl(single, (lane + 16 * d) & 63, 64);
        }
        if (q >= Q) continue;
        const bool cont_in = h > 0 && gF >= 0 && gLp == gF;  // the first run started in an earlier lane
        if (!single && !cont_in) atomicMax(Fq + gF, bF);
        if (gL >= 0 && !(single && cont_in)) {
            uint32_t total = bL;
#pragma unroll
            for (int d = 1; d <= 3; ++d) {
                if (h + d > 3 || gFn[d - 1] != gL) break;
                total = bFn[d - 1] > total ? bFn[d - 1] : total;
                if (!sn[d - 1]) break;
            }
            atomicMax(Fq + gL, total);
        }
    }
}

// ---- select: the radix path ----------------------------------------------------------------------------------------
// One block per query: the best `take` = min(M + 1, ng) groups by (fp32 max desc, group asc) over ALL groups.  Four
// 8-bit radix passes find the take-th largest key T; then one ordered pass collects every key > T and the first needed
// keys == T.  The overflow path of the select.
__device__ void radix_select_all(const uint32_t *__restrict__ Fq, int ng, int take, int *__restrict__ og,
                                 uint32_t *__restrict__ ok) {
    __shared__ int hist[256];
    __shared__ uint32_t prefix_sh;
    __shared__ int need_sh, wcnt[SEL_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t prefix = 0, mask = 0;
    int need = take;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int b = tid; b < 256; b += SEL_THREADS) hist[b] = 0;
        __syncthreads();
        for (int i = tid; i < ng; i += SEL_THREADS) {
            const uint32_t v = Fq[i];
            if ((v & mask) == prefix) atomicAdd(&hist[(v >> shift) & 255], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int above = 0;
            for (int b = 255; b >= 0; --b) {
                if (above + hist[b] >= need) {
                    need_sh = need - above;
                    prefix_sh = prefix | ((uint32_t)b << shift);
                    break;
                }
                above += hist[b];
            }
        }
        __syncthreads();
        prefix = prefix_sh;
        need = need_sh;
        mask |= 255u << shift;
    }
    // keys > T go to [0, take - need) in any order, keys == T to [take - need, take) in group order
    const uint32_t T = prefix;
    const int n_gt = take - need;
    __shared__ int gt_pos;
    if (tid == 0) gt_pos = 0;
    __syncthreads();
    int eq_base = 0;
    for (int c0 = 0; c0 < ng; c0 += SEL_THREADS) {
        const int i = c0 + tid;
        const uint32_t v = i < ng ? Fq[i] : 0;
        const bool gt = i < ng && v > T, eq = i < ng && v == T;
        if (gt) {
            const int pos = atomicAdd(&gt_pos, 1);
            og[pos] = i;
            ok[pos] = v;
        }
        const unsigned long long bal = __ballot(eq);
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int before = eq_base, total = 0;
        for (int w = 0; w < SEL_THREADS / 64; ++w) {
            if (w < wave) before += wcnt[w];
            total += wcnt[w];
        }
        before += __popcll(bal & ((1ull << lane) - 1ull));
        if (eq && before < need) {
            og[n_gt + before] = i;
            ok[n_gt + before] = v;
        }
        eq_base += total;
        const bool done = eq_base >= need && gt_pos == n_gt;  // uniform: read after the barrier below
        __syncthreads();
        if (done) break;
    }
}

// ---- finalize ----------------------------------------------------------------------------------------------
// SC, here and in the redo: the row predicate (vm_internal.h) - NoScope (the grouped search) or TagScope (the scoped
// grouped search).  Passed to the two kernels by value; every use of it sits under `if constexpr (SC::scoped)`, so the
// grouped search's instantiations keep the instructions they had.
constexpr int GF_OUT = 255;  // the candidate index of an out-of-scope row (candidates are < GCMAX)

// One block per query.  Ranks the take candidates by (fp32 key desc, group asc): the first nc = min(take, M) are
// re-scored, the (M+1)-th (if any) bounds every rejected group.  Every row of a candidate group is scored exactly
// (a row whose fp32 score is more than 2 eps below its group's fp32 max can not be the max, but the rows of a
// candidate group are few and scoring them all needs no per-row fp32 score), exact max and lowest row reaching it by
// LDS atomics, then the k best by (score desc, representative asc).
template <int DT, class SC>
__global__ void __launch_bounds__(GF_THREADS)
    group_finalize_kernel(const uint16_t *__restrict__ mem, const double *__restrict__ norm64,
                          const int64_t *__restrict__ gkey, const int64_t *__restrict__ gord,
                          const uint16_t *__restrict__ queries, const int64_t *__restrict__ d_total, int64_t cap,
                          int ring, int D, const int *__restrict__ first_o, const int *__restrict__ cand_g,
                          const uint32_t *__restrict__ cand_k, const int *__restrict__ cand_n, int M, int k, int use_min,
                          double min_score, int score_mode, double *__restrict__ out_scores,
                          int64_t *__restrict__ out_rows, int64_t *__restrict__ out_keys, int *__restrict__ uncertified,
                          int *__restrict__ flags, int *__restrict__ user_flags, const SC sc) {
    extern __shared__ __attribute__((aligned(16))) char gf_dyn[];
    uint16_t *ql = reinterpret_cast<uint16_t *>(gf_dyn);  // [D]
    __shared__ int sg[GCMAX], ca[GCMAX], cpre[GCMAX + 1], rk[GCMAX], lg[GCMAX];
    __shared__ uint32_t sk[GCMAX], lk[GCMAX];
    __shared__ unsigned long long gmax[GCMAX];
    __shared__ long long grep[GCMAX];
    __shared__ double es[GROWCAP];
    __shared__ uint8_t ec[GROWCAP];
    __shared__ double qn_sh;
    __shared__ int flag_sh;
    const int q = blockIdx.x, tid = threadIdx.x;
    const GroupView gv = group_view(d_total, cap, ring, gord);
    const typename SC::Q sq = sc.at(q);
    const int C = cand_n[q];
    const int nc = C < M ? C : M;
    for (int i = tid; i < D / 8; i += GF_THREADS)
        reinterpret_cast<uint4 *>(ql)[i] = reinterpret_cast<const uint4 *>(queries + (size_t)q * D)[i];
    if (tid < C) {
        lg[tid] = cand_g[(size_t)q * GCMAX + tid];
        lk[tid] = cand_k[(size_t)q * GCMAX + tid];
    }
    if (tid == 0) flag_sh = VM_FLAG_CERTIFIED;
    __syncthreads();
    if (tid < C) {  // rank by (fp32 key desc, group asc)
        const int g = lg[tid];
        const uint32_t key = lk[tid];
        int r = 0;
        for (int j = 0; j < C; ++j) r += (lk[j] > key || (lk[j] == key && lg[j] < g)) ? 1 : 0;
        sg[r] = g;
        sk[r] = key;
    }
    __syncthreads();
    if (tid < nc) {
        const int a = first_o[sg[tid]];
        ca[tid] = a;
        cpre[tid + 1] = first_o[sg[tid] + 1] - a;  // length for now
        gmax[tid] = 0;
        grep[tid] = LLONG_MAX;
    }
    if (tid == 64) qn_sh = exact_qnorm<DT>(ql, D);  // the second wave; the prefix sum below is the first's
    __syncthreads();
    if (tid == 0) {
        cpre[0] = 0;
        for (int c = 0; c < nc; ++c) cpre[c + 1] += cpre[c];
    }
    __syncthreads();
    const int R = cpre[nc];
    const double qn = qn_sh;
    if (R > GROWCAP) {  // uniform: too many candidate rows -> the exhaustive redo answers this query
        for (int i = tid; i < k; i += GF_THREADS) {
            out_scores[(size_t)q * k + i] = 0.0;
            out_rows[(size_t)q * k + i] = -1;
            if (out_keys) out_keys[(size_t)q * k + i] = -1;
        }
        if (tid == 0) {
            flags[q] = VM_FLAG_OVERFLOW;
            if (user_flags) user_flags[q] = VM_FLAG_OVERFLOW;
            if (uncertified) atomicAdd(uncertified, 1);
        }
        return;
    }
    for (int r = tid; r < R; r += GF_THREADS) {
        int lo = 0, hi = nc - 1;  // the candidate c with cpre[c] <= r < cpre[c + 1]
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (cpre[mid] <= r) lo = mid;
            else hi = mid - 1;
        }
        const int64_t o = ca[lo] + (r - cpre[lo]);
        if constexpr (SC::scoped) {
            if (!sq.in(slot_of(gv.rv, o))) {  // an out-of-scope row of a candidate group: not scored, in no max
                ec[r] = GF_OUT;
                continue;
            }
        }
        const double e = exact_score<DT>(ql, qn, mem, norm64, slot_of(gv.rv, o), D);
        es[r] = e;
        ec[r] = (uint8_t)lo;
        atomicMax(&gmax[lo], okey64(e));
    }
    __syncthreads();
    for (int r = tid; r < R; r += GF_THREADS) {
        const int c = ec[r];
        if constexpr (SC::scoped) {
            if (c == GF_OUT) continue;
        }
        if (okey64(es[r]) == gmax[c]) atomicMin(&grep[c], (long long)(ca[c] + (r - cpre[c])));
    }
    __syncthreads();
    if (tid < nc) {
        const double e = dekey64(gmax[tid]);
        const long long o = grep[tid];
        int r = 0;
        for (int d = 0; d < nc; ++d) {
            const double e2 = dekey64(gmax[d]);
            r += (e2 > e || (e2 == e && grep[d] < o)) ? 1 : 0;
        }
        rk[tid] = r;
        if (r < k) {
            const double shown = shown_score(e, score_mode);
            const bool pass = passes_min(use_min, shown, min_score);
            out_scores[(size_t)q * k + r] = pass ? shown : 0.0;
            out_rows[(size_t)q * k + r] = pass ? gv.rv.base + o : -1;
            if (out_keys) out_keys[(size_t)q * k + r] = pass ? gkey[slot_of(gv.rv, o)] : -1;
        }
        // certification: the exact k-th group score against the best fp32 max of a group that never became a candidate
        const int kth = (k < nc ? k : nc) - 1;
        // (clears_gap of topk_select.h written out: called as a helper it changes this kernel's instructions)
        if (r == kth && C > M && qn != 0.0) {
            const double eps = cert_eps(D);
            const double reject = (double)dekey32(sk[M]) / qn + eps;
            if (!(e > reject)) flag_sh = VM_FLAG_GAP;
        }
    }
    for (int i = nc + tid; i < k; i += GF_THREADS) {
        out_scores[(size_t)q * k + i] = 0.0;
        out_rows[(size_t)q * k + i] = -1;
        if (out_keys) out_keys[(size_t)q * k + i] = -1;
    }
    __syncthreads();
    if (tid == 0) {
        int f = flag_sh;
        // domain of the certificate (topk_common.h cert_eps; bf16 only): outside it the in-call redo answers the query
        if constexpr (DT == VM_BF16) {
            if (f == VM_FLAG_CERTIFIED && gv.rv.n > 0 && (d_total[VM_GSTATE_OUTSIDE] != 0 || cert_norm_outside(qn)))
                f = VM_FLAG_GAP;
        }
        flags[q] = f;
        if (user_flags) user_flags[q] = f;
        if (f && uncertified) atomicAdd(uncertified, 1);
    }
}

// ---- redo --------------------------------------------------------------------------------------------------
// grid = nblk.  Block b owns the groups whose first live row lies in its even slice [lo, hi) of age orders, so every
// group is scored whole by one block (a group longer than a slice makes its block longer).  Per flagged query: rows in
// chunks of GR_CHUNK, exact scores, per-chunk group max + lowest row by LDS atomics, the chunk's last group carried into
// the next chunk, and a stable top-k of complete groups: part[(b * Q + q) * k + i] = {score, representative order}.
template <int DT, class SC>
__global__ void __launch_bounds__(GR_THREADS)
    group_redo_scan_kernel(const uint16_t *__restrict__ queries, const uint16_t *__restrict__ mem,
                           const double *__restrict__ norm64, const int64_t *__restrict__ gord,
                           const int64_t *__restrict__ d_total, int64_t cap, int ring, int D, int Q, int k,
                           const int *__restrict__ first_o, const int32_t *__restrict__ flags,
                           double *__restrict__ part_s, int64_t *__restrict__ part_o, const SC sc) {
    extern __shared__ __attribute__((aligned(16))) char gr_dyn[];
    uint16_t *ql = reinterpret_cast<uint16_t *>(gr_dyn);  // [D]
    __shared__ double rs[GR_CHUNK];
    __shared__ short lidx[GR_CHUNK];
    __shared__ unsigned long long gmax[GR_CHUNK];
    __shared__ long long grep[GR_CHUNK];
    __shared__ double run_s[GKMAX], new_s[GKMAX], red_s[GR_THREADS / 64];
    __shared__ int64_t run_o[GKMAX], new_o[GKMAX], red_o[GR_THREADS / 64];
    __shared__ double qn_sh, carry_s;
    __shared__ int64_t carry_o, carry_g;
    __shared__ int carry_live, r0_sh, r1_sh;
    const int tid = threadIdx.x;
    int any = 0;
    for (int i = tid; i < Q; i += GR_THREADS) any |= flags[i];
    if (!__syncthreads_or(any)) return;
    const GroupView gv = group_view(d_total, cap, ring, gord);
    const int64_t n = gv.rv.n;
    if (tid == 0) {
        const int64_t per = (n + gridDim.x - 1) / gridDim.x;
        int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per;
        lo = lo < n ? lo : n;
        hi = hi < n ? hi : n;
        // first group whose first row is >= x: first_o is increasing over [0, ng] with first_o[ng] = n
        auto lower = [&](int64_t x) {
            int64_t a = 0, b = gv.ng;
            while (a < b) {
                const int64_t mid = (a + b) >> 1;
                if (first_o[mid] < x) a = mid + 1;
                else b = mid;
            }
            return first_o[a];
        };
        r0_sh = (int)lower(lo);
        r1_sh = (int)lower(hi);
    }
    __syncthreads();
    const int64_t r0 = r0_sh, r1 = r1_sh;
    for (int q = 0; q < Q; ++q) {
        if (flags[q] == 0) continue;  // uniform
        __syncthreads();
        for (int i = tid; i < D / 8; i += GR_THREADS)
            reinterpret_cast<uint4 *>(ql)[i] = reinterpret_cast<const uint4 *>(queries + (size_t)q * D)[i];
        if (tid < k) {
            run_s[tid] = -INFINITY;
            run_o[tid] = -1;
        }
        if (tid == 0) carry_live = 0;
        __syncthreads();
        if (tid == 0) qn_sh = exact_qnorm<DT>(ql, D);
        __syncthreads();
        const double qn = qn_sh;
        const typename SC::Q sq = sc.at(q);
        for (int64_t c0 = r0; c0 < r1; c0 += GR_CHUNK) {
            const int cn = (int)(r1 - c0 < GR_CHUNK ? r1 - c0 : GR_CHUNK);
            const bool last_chunk = c0 + cn >= r1;
            const int64_t gbase = gord[slot_of(gv.rv, c0)] - gv.ord0;
            for (int i = tid; i < cn; i += GR_THREADS) {
                gmax[i] = 0;
                grep[i] = LLONG_MAX;
            }
            __syncthreads();
            for (int i = tid; i < cn; i += GR_THREADS) {
                const int64_t p = slot_of(gv.rv, c0 + i);
                if constexpr (SC::scoped) {
                    if (!sq.in(p)) {  // out of scope: raises no max, and -inf is below every score, so it equals none
                        rs[i] = -INFINITY;
                        lidx[i] = (short)(gord[p] - gv.ord0 - gbase);
                        continue;
                    }
                }
                const double e = exact_score<DT>(ql, qn, mem, norm64, p, D);
                const int li = (int)(gord[p] - gv.ord0 - gbase);
                rs[i] = e;
                lidx[i] = (short)li;
                atomicMax(&gmax[li], okey64(e));
            }
            __syncthreads();
            for (int i = tid; i < cn; i += GR_THREADS)
                if (okey64(rs[i]) == gmax[lidx[i]]) atomicMin(&grep[lidx[i]], (long long)(c0 + i));
            __syncthreads();
            const int nl = lidx[cn - 1] + 1;
            __shared__ int carry_cand;
            if (tid == 0) {
                carry_cand = 0;
                if (carry_live) {
                    if (carry_g == gbase) {  // the carried group goes on in this chunk: its earlier rows win ties
                        if ((!SC::scoped || carry_o != LLONG_MAX) && okey64(carry_s) >= gmax[0]) {
                            gmax[0] = okey64(carry_s);
                            grep[0] = carry_o;
                        }
                    } else {
                        carry_cand = 1;
                    }
                }
            }
            __syncthreads();
            const int nloc = last_chunk ? nl : nl - 1;
            const int ncar = carry_cand;
            block_select<GR_THREADS>(nloc + ncar + k, k,
                          [&](int i, double &v, int64_t &o) {
                              if (i < nloc) {
                                  v = dekey64(gmax[i]);
                                  o = grep[i];
                              } else if (i < nloc + ncar) {
                                  v = carry_s;
                                  o = carry_o;
                              } else {
                                  v = run_s[i - nloc - ncar];
                                  o = run_o[i - nloc - ncar];
                              }
                              if constexpr (SC::scoped) {  // a group with no in-scope row is no group for this query
                                  if (o == LLONG_MAX) o = -1;
                              }
                          },
                          new_s, new_o, red_s, red_o);
            if (tid < k) {
                run_s[tid] = new_s[tid];
                run_o[tid] = new_o[tid];
            }
            if (tid == 0) {
                carry_live = last_chunk ? 0 : 1;
                if (!last_chunk) {
                    carry_s = dekey64(gmax[nl - 1]);
                    carry_o = grep[nl - 1];
                    carry_g = gbase + nl - 1;
                }
            }
            __syncthreads();
        }
        if (tid < k) {
            part_s[((size_t)blockIdx.x * Q + q) * k + tid] = run_s[tid];
            part_o[((size_t)blockIdx.x * Q + q) * k + tid] = run_o[tid];
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------
struct GPlan : TopkGeom {
    int tbl_blocks;
    size_t off_first, off_cg, off_ck, off_cn, off_flags, off_ps, off_po, off_cut, off_cc, off_cbuf, total;
};

GPlan group_plan(const vm_memory *m, int Q, int k) {
    GPlan p;
    static_cast<TopkGeom &>(p) = vm_topk_geom(m, Q, k, TS_THREADS, GR_CHUNK);
    int64_t tb = (m->cap + 256) / 256;
    p.tbl_blocks = (int)(tb < 1024 ? tb : 1024);
    WsBump ws;
    ws.take((size_t)Q * (size_t)m->cap * 4);  // F at offset 0: [Q][live groups] fp32-max keys
    p.off_first = ws.take((size_t)(m->cap + 1) * 4);
    p.off_cg = ws.take((size_t)Q * GCMAX * 4);
    p.off_ck = ws.take((size_t)Q * GCMAX * 4);
    p.off_cn = ws.take((size_t)Q * 4);
    p.off_flags = ws.take((size_t)Q * 4);
    p.off_cut = ws.take((size_t)Q * 8);
    p.off_cc = ws.take((size_t)Q * 4);
    p.off_cbuf = ws.take((size_t)Q * SEL_CAP * 8);
    p.off_ps = ws.take((size_t)p.nblk * Q * k * 8);
    p.off_po = ws.take((size_t)p.nblk * Q * k * 8);
    p.total = ws.off;
    return p;
}

// ---- host: the one driver of the two grouped searches -------------------------------------------------------
// what every entry point of a grouped search is called with, past the operands of its predicate (vidmem.h: group
// searches return row ids as they are, so row_stride = 1 and row_offset = 0)
struct GroupCall {
    const void *queries;
    int Q, k, use_min;
    double min_score;
    int score_mode;
    double *out_scores;
    int64_t *out_rows, *out_keys;
    int32_t *out_uncertified, *out_query_flags;  // null in the exhaustive-only entry points
    char *ws;
    hipStream_t stream;
};

// redo: flagged queries scored exhaustively, whole groups per block, then the one merge of every redo, with keys
template <int DT, class SC>
int grouped_redo(vm_memory *m, const GPlan &p, const GroupCall &c, const SC &sc) {
    vm_ctx *ctx = m->ctx;
    vm_prof_scope prof(ctx, VM_PROF_TOPK_EXACT, c.stream);
    const int *first_o = (const int *)(c.ws + p.off_first);
    const int32_t *flags = (const int32_t *)(c.ws + p.off_flags);
    double *part_s = (double *)(c.ws + p.off_ps);
    int64_t *part_o = (int64_t *)(c.ws + p.off_po);
    group_redo_scan_kernel<DT, SC><<<p.nblk, GR_THREADS, (size_t)m->D * 2, c.stream>>>(
        (const uint16_t *)c.queries, m->rows, m->norm64, m->gord, m->d_total, m->cap, m->ring, m->D, c.Q, c.k, first_o,
        flags, part_s, part_o, sc);
    VM_LAUNCH_CHECK(ctx);
    return vm_topk_redo_merge(m, part_s, part_o, p.nblk, c.Q, c.k, flags, c.use_min, c.min_score, c.score_mode, 1, 0,
                              c.out_scores, c.out_rows, m->gkey, c.out_keys, c.stream);
}

// table -> scan -> cut -> compact -> select -> finalize -> redo.  Scan: the tile-scan policy that raises the group maxima
// (its Args have F, the plan's, filled in here); Cut / SelectFinal: the search's two select kernels, which differ in what
// an empty group is (topk_group.hip, topk_group_scope.hip) and stay two because merged they compile to other
// instructions; sc: the row predicate of the finalize and the redo.
template <int DT, class Scan, auto Cut, auto SelectFinal, class SC>
int grouped_topk(vm_memory *m, const GroupCall &c, typename Scan::Args a, const SC &sc) {
    vm_ctx *ctx = m->ctx;
    hipStream_t st = c.stream;
    char *ws = c.ws;
    const int Q = c.Q;
    const GPlan p = group_plan(m, Q, c.k);
    uint32_t *F = (uint32_t *)ws;
    int *first_o = (int *)(ws + p.off_first);
    int *cand_g = (int *)(ws + p.off_cg);
    uint32_t *cand_k = (uint32_t *)(ws + p.off_ck);
    int *cand_n = (int *)(ws + p.off_cn);
    int *flags = (int *)(ws + p.off_flags);
    {
        vm_prof_scope prof(ctx, VM_PROF_TOPK_SCAN, st);
        if (int rc = vm_group_table(m, p.tbl_blocks, Q, first_o, F, nullptr, 0, st)) return rc;
        a.F = F;
        const int rc = vm_tile_scan<DT, Scan>(m, p, c.queries, Q, a, st);
        if (rc != VM_OK) return rc;
    }
    {
        vm_prof_scope prof(ctx, VM_PROF_TOPK_FINALIZE, st);
        unsigned long long *cut = (unsigned long long *)(ws + p.off_cut);
        int *ccount = (int *)(ws + p.off_cc);
        unsigned long long *cbuf = (unsigned long long *)(ws + p.off_cbuf);
        Cut<<<Q, SEL_THREADS, 0, st>>>(m->d_total, m->cap, m->ring, m->gord, F, p.M + 1, cut, ccount);
        VM_LAUNCH_CHECK(ctx);
        if (int rc = vm_group_compact(m, p.cmp_slices, Q, F, cut, ccount, cbuf, st)) return rc;
        SelectFinal<<<Q, SEL_THREADS, 0, st>>>(m->d_total, m->cap, m->ring, m->gord, F, p.M + 1, ccount, cbuf, cand_g,
                                               cand_k, cand_n);
        VM_LAUNCH_CHECK(ctx);
        group_finalize_kernel<DT, SC><<<Q, GF_THREADS, (size_t)m->D * 2, st>>>(
            m->rows, m->norm64, m->gkey, m->gord, (const uint16_t *)c.queries, m->d_total, m->cap, m->ring, m->D, first_o,
            cand_g, cand_k, cand_n, p.M, c.k, c.use_min, c.min_score, c.score_mode, c.out_scores, c.out_rows, c.out_keys,
            c.out_uncertified, flags, c.out_query_flags, sc);
        VM_LAUNCH_CHECK(ctx);
    }
    return grouped_redo<DT>(m, p, c, sc);
}

// the exhaustive-only entry point: the table with every query flagged, then the redo
template <class SC>
int grouped_exact(vm_memory *m, const GroupCall &c, const SC &sc) {
    const GPlan p = group_plan(m, c.Q, c.k);
    if (int rc = vm_group_table(m, p.tbl_blocks, c.Q, (int *)(c.ws + p.off_first), nullptr,
                                (int32_t *)(c.ws + p.off_flags), 1, c.stream))
        return rc;
    return vm_by_dtype(m, [&](auto dt) { return grouped_redo<decltype(dt)::value>(m, p, c, sc); });
}

}  // namespace
