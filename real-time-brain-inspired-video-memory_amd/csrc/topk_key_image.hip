// The select stage and the finalize of the key-image searches (topk_scope_select.h), compiled once: the kernels over one
// fp32 key per (query, physical slot), the workspace plan and the launches the scoped, masked, span, mixed and clip searches
// call.  The kernels stay in this unit's anonymous namespace; only the host functions are visible.
#include "topk_scope_select.h"

namespace {

constexpr int SEL_THREADS = 1024;  // cut and selection (one block per query)
constexpr int SEL_SAMPLE = 16384;  // slots whose keys give each query's cut
constexpr int CMP_THREADS = 256;   // compaction
constexpr int CMP_LCAP = 2048;     // hits one compaction block gathers in LDS before it flushes them

// ---- select ------------------------------------------------------------------------------------------------
// composites (topk_select.h) of key and age order: ties at one key go to the older row
// One block per query: cut[q] = the (M+1)-th largest key of a sample of SEL_SAMPLE slots, one per stride (all slots when
// there are fewer), or 1 - every in-scope row - when the sample holds fewer than M + 1 in-scope rows.  At least
// min(M + 1, in-scope rows) rows have a key >= the cut, and no out-of-scope row (key 0) has.
__global__ void __launch_bounds__(SEL_THREADS)
    scope_cut_kernel(const int64_t *__restrict__ d_total, int64_t cap, int ring, const uint32_t *__restrict__ F,
                     int64_t fstride, int M1, uint32_t *__restrict__ cut, int *__restrict__ ccount) {
    constexpr int PER = SEL_SAMPLE / SEL_THREADS;
    const int q = blockIdx.x, tid = threadIdx.x;
    const int64_t n = ring_view(*d_total, cap, ring).n;
    const uint32_t *Fq = F + (size_t)q * fstride;
    const int cnt = (int)(n < SEL_SAMPLE ? n : SEL_SAMPLE);
    uint32_t v[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = j * SEL_THREADS + tid;
        // one slot per stride, at a hashed offset inside it: a fixed stride of 64 slots would see one source only of
        // two that alternate every 16 rows
        int64_t p = i;
        if (n > SEL_SAMPLE) p = (int64_t)i * n / SEL_SAMPLE + (int64_t)(((uint32_t)i * 2654435761u) >> 8) % (n / SEL_SAMPLE);
        v[j] = i < cnt ? Fq[p] : 0u;
    }
    // the top 20 bits of the key are enough for a cut (a score resolution of 2^-11 relative): 20 counting steps, not 32.
    // 0 when fewer than M1 sampled keys are in scope (every in-scope key is above 2^12)
    const uint32_t T = block_kth_u32<SEL_THREADS>(v, M1, 12);
    if (tid == 0) {
        cut[q] = T ? T : 1u;
        ccount[q] = 0;
    }
}

// grid (slices, Q): every in-scope row with key >= cut[q] goes to the query's buffer as a composite.  Hits gather in
// LDS and leave with one global atomic per flush.  ccount[q] ends as the exact number of hits; the buffer keeps the
// first SEL_CAP.
__global__ void __launch_bounds__(CMP_THREADS)
    scope_compact_kernel(const int64_t *__restrict__ d_total, int64_t cap, int ring, const uint32_t *__restrict__ F,
                         int64_t fstride, const uint32_t *__restrict__ cut, int *__restrict__ ccount,
                         unsigned long long *__restrict__ cbuf) {
    __shared__ unsigned long long lbuf[CMP_LCAP];
    __shared__ int lcnt, gbase;
    const int q = blockIdx.y, tid = threadIdx.x;
    const RingView rv = ring_view(*d_total, cap, ring);
    const int64_t n = rv.n;
    const uint32_t *Fq = F + (size_t)q * fstride;
    const uint32_t T = cut[q];
    const int64_t stride = (int64_t)gridDim.x * CMP_THREADS * 4;
    if (tid == 0) lcnt = 0;
    __syncthreads();
    int held_max = 0;  // block-uniform upper bound of the hits in lbuf
    auto flush = [&]() {  // called by every thread
        __syncthreads();  // every hit of the iterations so far is in lbuf and counted in lcnt
        const int held = lcnt;
        if (tid == 0 && held) gbase = atomicAdd(&ccount[q], held);
        __syncthreads();
        for (int i = tid; i < held; i += CMP_THREADS) {
            const int pos = gbase + i;
            if (pos < SEL_CAP) cbuf[(size_t)q * SEL_CAP + pos] = lbuf[i];
        }
        __syncthreads();
        if (tid == 0) lcnt = 0;
        held_max = 0;
        __syncthreads();
    };
    for (int64_t base = (int64_t)blockIdx.x * CMP_THREADS * 4; base < n; base += stride) {  // uniform per block
        const int64_t p = base + 4 * tid;  // 4 consecutive slots, 16-byte aligned (fstride is a multiple of 64)
        uint4 k4 = make_uint4(0, 0, 0, 0);
        if (p < n) k4 = *reinterpret_cast<const uint4 *>(Fq + p);
        const uint32_t key[4] = {k4.x, k4.y, k4.z, k4.w};
        int hits = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) hits += (p + j < n && key[j] >= T) ? 1 : 0;  // T >= 1: never an out-of-scope row
        if (hits) {  // rare: one LDS atomic per thread with hits
            int pos = atomicAdd(&lcnt, hits);  // pos + hits <= CMP_LCAP: flushed before it could fill
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (p + j < n && key[j] >= T) lbuf[pos++] = composite(key[j], (int)order_of(rv, p + j));
        }
        held_max += 4 * __syncthreads_count(hits != 0);
        if (held_max > CMP_LCAP - 4 * CMP_THREADS) flush();
    }
    flush();
}

// One block per query: the best take = min(M + 1, hits) composites of the compacted list.  cand_n[q] = take, or -1 when
// the list overflowed (the finalize flags the query for the exhaustive redo).
__global__ void __launch_bounds__(SEL_THREADS)
    scope_select_kernel(int M1, const int *__restrict__ ccount, const unsigned long long *__restrict__ cbuf,
                        int *__restrict__ cand_o, uint32_t *__restrict__ cand_k, int *__restrict__ cand_n) {
    const int q = blockIdx.x, tid = threadIdx.x;
    int *oo = cand_o + (size_t)q * SCMAX;
    uint32_t *ok = cand_k + (size_t)q * SCMAX;
    const int cnt = ccount[q];
    if (cnt > SEL_CAP || cnt == 0) {  // uniform
        if (tid == 0) cand_n[q] = cnt ? -1 : 0;
        return;
    }
    const int take = cnt < M1 ? cnt : M1;
    if (tid == 0) cand_n[q] = take;
    select_best<SEL_THREADS, SEL_CAP, SCMAX>(cbuf + (size_t)q * SEL_CAP, cnt, take, oo, ok);
}

// ---- finalize ----------------------------------------------------------------------------------------------
// One block per query.  Ranks the C candidates by (fp32 key desc, order asc): the first nc = min(C, M) are re-scored
// exactly, the (M+1)-th (if any) bounds every other in-scope row.  "In scope" = has a nonzero key: nothing here knows
// whether a tag range or a mask bit made it so.
template <int DT>
__global__ void __launch_bounds__(SF_THREADS)
    scope_finalize_kernel(const uint16_t *__restrict__ mem, const double *__restrict__ norm64,
                          const uint16_t *__restrict__ queries, const int64_t *__restrict__ d_total, int64_t cap,
                          int ring, int D, const int *__restrict__ cand_o, const uint32_t *__restrict__ cand_k,
                          const int *__restrict__ cand_n, int M, int k, int use_min, double min_score, int score_mode,
                          int64_t row_stride, int64_t row_offset, double *__restrict__ out_scores,
                          int64_t *__restrict__ out_rows, int *__restrict__ uncertified, int *__restrict__ flags,
                          int *__restrict__ user_flags) {
    extern __shared__ __attribute__((aligned(16))) char sf_dyn[];
    uint16_t *ql = reinterpret_cast<uint16_t *>(sf_dyn);  // [D]
    __shared__ int so[SCMAX], lo_[SCMAX];
    __shared__ uint32_t sk[SCMAX], lk[SCMAX];
    __shared__ double es[SCMAX];
    __shared__ double qn_sh;
    __shared__ int flag_sh;
    const int q = blockIdx.x, tid = threadIdx.x;
    const RingView rv = ring_view(*d_total, cap, ring);
    const int C = cand_n[q];
    if (C < 0) {  // uniform: more rows at the cut than the buffer holds -> the exhaustive redo answers this query
        for (int i = tid; i < k; i += SF_THREADS) {
            out_scores[(size_t)q * k + i] = 0.0;
            out_rows[(size_t)q * k + i] = -1;
        }
        if (tid == 0) {
            flags[q] = VM_FLAG_OVERFLOW;
            if (user_flags) user_flags[q] = VM_FLAG_OVERFLOW;
            if (uncertified) atomicAdd(uncertified, 1);
        }
        return;
    }
    const int nc = C < M ? C : M;
    for (int i = tid; i < D / 8; i += SF_THREADS)
        reinterpret_cast<uint4 *>(ql)[i] = reinterpret_cast<const uint4 *>(queries + (size_t)q * D)[i];
    if (tid < C) {
        lo_[tid] = cand_o[(size_t)q * SCMAX + tid];
        lk[tid] = cand_k[(size_t)q * SCMAX + tid];
    }
    if (tid == 0) flag_sh = VM_FLAG_CERTIFIED;
    __syncthreads();
    if (tid < C) {  // rank by (fp32 key desc, order asc)
        const int o = lo_[tid];
        const uint32_t key = lk[tid];
        int r = 0;
        for (int j = 0; j < C; ++j) r += (lk[j] > key || (lk[j] == key && lo_[j] < o)) ? 1 : 0;
        so[r] = o;
        sk[r] = key;
    }
    if (tid == SF_THREADS - 1) qn_sh = __dsqrt_rn(ref_sumsq<DT>(ql, D));
    __syncthreads();
    const double qn = qn_sh;
    if (tid < nc) {
        const int64_t p = slot_of(rv, so[tid]);
        es[tid] = ref_cosine(ref_dot<DT>(ql, mem + (size_t)p * D, D), qn, norm64[p]);
    }
    __syncthreads();
    if (tid < nc) {
        const double e = es[tid];
        const int o = so[tid];
        int r = 0;
        for (int d = 0; d < nc; ++d) r += (es[d] > e || (es[d] == e && so[d] < o)) ? 1 : 0;
        if (r < k) {
            const double shown = shown_score(e, score_mode);
            const bool pass = passes_min(use_min, shown, min_score);
            out_scores[(size_t)q * k + r] = pass ? shown : 0.0;
            out_rows[(size_t)q * k + r] = pass ? (rv.base + o) * row_stride + row_offset : -1;
        }
        // certification: the exact k-th score against the best fp32 score of an in-scope row that was not re-scored
        const int kth = (k < nc ? k : nc) - 1;
        if (r == kth && C > M && qn != 0.0 && !clears_gap(e, sk[M], qn, D)) flag_sh = VM_FLAG_GAP;
    }
    for (int i = nc + tid; i < k; i += SF_THREADS) {
        out_scores[(size_t)q * k + i] = 0.0;
        out_rows[(size_t)q * k + i] = -1;
    }
    __syncthreads();
    if (tid == 0) {
        int f = flag_sh;
        // domain of the certificate (topk_common.h cert_eps; bf16 only): outside it the in-call redo answers the query
        if constexpr (DT == VM_BF16) {
            if (f == VM_FLAG_CERTIFIED && rv.n > 0 && (d_total[VM_GSTATE_OUTSIDE] != 0 || cert_norm_outside(qn)))
                f = VM_FLAG_GAP;
        }
        flags[q] = f;
        if (user_flags) user_flags[q] = f;
        if (f && uncertified) atomicAdd(uncertified, 1);
    }
}

__global__ void fill_flags_kernel(int32_t *__restrict__ flags, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flags[i] = 1;
}

}  // namespace

// ---- host --------------------------------------------------------------------------------------------------
SPlan vm_key_image_plan(const vm_memory *m, int Q, int k) {
    SPlan p;
    static_cast<TopkGeom &>(p) = vm_topk_geom(m, Q, k, TS_THREADS, VM_REDO_CHUNK_SCOPED);
    p.fstride = (m->cap + 63) / 64 * 64;  // the columns' padding: a tail tile writes its 16 keys
    WsBump ws;
    ws.take((size_t)Q * (size_t)p.fstride * 4);  // F at offset 0: [Q][slot] fp32 keys
    p.off_co = ws.take((size_t)Q * SCMAX * 4);
    p.off_ck = ws.take((size_t)Q * SCMAX * 4);
    p.off_cn = ws.take((size_t)Q * 4);
    p.off_flags = ws.take((size_t)Q * 4);
    p.off_cut = ws.take((size_t)Q * 4);
    p.off_cc = ws.take((size_t)Q * 4);
    p.off_cbuf = ws.take((size_t)Q * SEL_CAP * 8);
    p.off_ps = ws.take((size_t)p.nblk * Q * k * 8);
    p.off_po = ws.take((size_t)p.nblk * Q * k * 8);
    p.total = ws.off;
    return p;
}

int vm_key_image_select(vm_memory *m, const SelectPlan &p, const uint32_t *F, int Q, char *ws, hipStream_t st) {
    vm_ctx *ctx = m->ctx;
    uint32_t *cut = (uint32_t *)(ws + p.off_cut);
    int *ccount = (int *)(ws + p.off_cc);
    unsigned long long *cbuf = (unsigned long long *)(ws + p.off_cbuf);
    scope_cut_kernel<<<Q, SEL_THREADS, 0, st>>>(m->d_total, m->cap, m->ring, F, p.fstride, p.M + 1, cut, ccount);
    VM_LAUNCH_CHECK(ctx);
    scope_compact_kernel<<<dim3(p.cmp_slices, Q), CMP_THREADS, 0, st>>>(m->d_total, m->cap, m->ring, F, p.fstride, cut,
                                                                        ccount, cbuf);
    VM_LAUNCH_CHECK(ctx);
    scope_select_kernel<<<Q, SEL_THREADS, 0, st>>>(p.M + 1, ccount, cbuf, (int *)(ws + p.off_co),
                                                   (uint32_t *)(ws + p.off_ck), (int *)(ws + p.off_cn));
    VM_LAUNCH_CHECK(ctx);
    return VM_OK;
}

int vm_key_image_finalize(vm_memory *m, const SPlan &p, const RowCall &c) {
    return vm_by_dtype(m, [&](auto dt) {
        scope_finalize_kernel<decltype(dt)::value><<<c.Q, SF_THREADS, (size_t)m->D * 2, c.stream>>>(
            m->rows, m->norm64, (const uint16_t *)c.queries, m->d_total, m->cap, m->ring, m->D,
            (const int *)(c.ws + p.off_co), (const uint32_t *)(c.ws + p.off_ck), (const int *)(c.ws + p.off_cn), p.M, c.k,
            c.use_min, c.min_score, c.score_mode, c.row_stride, c.row_offset, c.out_scores, c.out_rows,
            c.out_uncertified, (int *)(c.ws + p.off_flags), c.out_query_flags);
        VM_LAUNCH_CHECK(m->ctx);
        return (int)VM_OK;
    });
}

int vm_fill_flags(vm_memory *m, int32_t *flags, int n, hipStream_t st) {
    fill_flags_kernel<<<(n + 255) / 256, 256, 0, st>>>(flags, n);
    VM_LAUNCH_CHECK(m->ctx);
    return VM_OK;
}
