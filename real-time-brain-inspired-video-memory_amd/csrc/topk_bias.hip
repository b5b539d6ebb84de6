// Biased cosine top-k: the k best rows by COSINE PLUS A PER-ROW PRIOR (include/vidmem.h vm_topk_cosine_biased), and the two
// device-side builders of such priors.  A bias column is one fp32 value per physical slot - recency, a decaying strength,
// a boost for the rows another retrieval leg found - and S(q, r) = e(q, r) + beta_q * b[slot(r)], e = the reference cosine,
// b widened exactly to fp64, one fp64 rounding for the product and one for the sum, never fused.
//
// The masked search (topk_mask.hip) with another score, built from the parts the mixed search (topk_mix.hip) is built from:
//   pack     : per query the fp64 norm, coef = fl32(1 / ||q||), g = fl32(beta), the offset of its bias column (-1 = the
//              zero column) and the flag of the bound's domain
//   scan     : topk_tile_scan.h under the BiasScan policy below, one query per MFMA column as in MaskScan.  The epilogue
//              reads the lane's four bias values with one 16-byte load next to the rows it has just scored:
//              F[q][slot] = okey32(B), B = fl32(fl32(coef * s) + fl32(g * b)), for a selected live row, 0 for any other
//   select   : topk_key_image.hip's vm_key_image_select as it is
//   finalize : bias_finalize_kernel: the exact S of the best M candidates; certified when at most M rows are selected or
//              the exact k-th S clears B* + eps_bias(D, B*), B* = dekey32(key of the (M+1)-th), strictly
//   redo     : bias_redo_scan_kernel (topk_redo_scan_kernel's structure, every admitted row scored exactly), then
//              vm_topk_redo_merge as it is
// Every launch reads the row count from the device and sizes its grid from the capacity: capturable.
#include "topk_scope_select.h"
#include "topk_tile_scan.h"

namespace {

constexpr int BIAS_THREADS = 256;  // finalize, redo
constexpr double BIAS_W_MIN = 9.5367431640625e-07;  // 2^-20: the weight domain of the bound, |beta| in [2^-20, 2^20] or 0
constexpr double BIAS_W_MAX = 1048576.0;            // 2^20
constexpr float BIAS_B_MAX = 1099511627776.f;       // 2^40: the bias domain of the bound, so g * b stays finite in fp32
constexpr int BIAS_Q_MAX = 1 << 20;                 // the workspace offsets stay far inside 32 bits of queries

// S of a memory: fp32 entries of one bias column, one per slot of the padded capacity (= 32 x mask_words)
inline int64_t bias_stride(const vm_memory *m) { return mask_words(m) * 32; }

// The bound of the scanned score B against the exact S inside the domain: the fp32 score times 1 / ||q||
// lies within cert_eps(D) of e; the roundings of coef, g, the two products and the sum cost at most 2^-24 relative each on
// magnitudes bounded by 1 + |beta b| <= 2 + |B| + the error itself: 4.2 x 2^-24 + 3.2 x 2^-24 |B|, stated with slack.
// B + eps_bias(D, B) is increasing in B (slope 1 +- 2^-22), so the bound at the (M+1)-th key covers every lower key.
__device__ __forceinline__ double eps_bias(int D, double B) {
    return __dadd_rn(__dadd_rn(cert_eps(D), 4.76837158203125e-07), __dmul_rn(2.384185791015625e-07, fabs(B)));
}

// the exact score: one rounding for the product, one for the sum
__device__ __forceinline__ double bias_exact(double e, double beta, float b) {
    return __dadd_rn(e, __dmul_rn(beta, (double)b));
}

// ---- pack --------------------------------------------------------------------------------------------------
// One wave per query; dynamic LDS: the query.  qn [Q] fp64 norms, coef / g [Q], boff [Q] the offset of the query's column
// in fp32 entries (-1: the zero column), dom [Q] the domain flag, which the scan ORs into.  The reference norm is one
// strictly ordered chain of D products and sums, so one lane computes it; the wave first brings the query into LDS with
// one coalesced read, or the chain would also wait for D / 8 dependent global loads (16.6 us against 9.8 us, measured at
// D = 768: this launch precedes the scan and nothing hides it).
template <int DT>
__global__ void __launch_bounds__(64)
    bias_pack_kernel(const uint16_t *__restrict__ queries, const double *__restrict__ weights,
                     const int32_t *__restrict__ bias_index, int n_bias, int64_t S, int Q, int D,
                     double *__restrict__ qn, float *__restrict__ coef, float *__restrict__ g,
                     int32_t *__restrict__ boff, int *__restrict__ dom) {
    extern __shared__ __attribute__((aligned(16))) char bp_dyn[];
    uint16_t *ql = reinterpret_cast<uint16_t *>(bp_dyn);  // [D]
    const int q = blockIdx.x;
    for (int i = threadIdx.x; i < D / 8; i += 64)
        reinterpret_cast<uint4 *>(ql)[i] = reinterpret_cast<const uint4 *>(queries + (size_t)q * D)[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double nrm = __dsqrt_rn(ref_sumsq<DT>(ql, D));
    const double beta = weights ? weights[q] : 1.0;
    const double a = fabs(beta);
    qn[q] = nrm;
    coef[q] = nrm == 0.0 ? 0.f : (float)__ddiv_rn(1.0, nrm);
    g[q] = (float)beta;
    const int64_t i = bias_index ? bias_index[q] : (n_bias == 1 ? 0 : q);
    boff[q] = i < 0 || i >= n_bias ? -1 : (int32_t)(i * S);  // below 2^30: the host refuses more bias values
    dom[q] = ((a != 0.0 && !(a >= BIAS_W_MIN && a <= BIAS_W_MAX)) || cert_norm_outside(nrm)) ? 1 : 0;
}

// ---- scan --------------------------------------------------------------------------------------------------
// The biased policy of the tile scan: MaskScan's keys with the score B = fl32(fl32(coef * s) + fl32(g * b)).
// ms.words == nullptr: no mask, every live row is selected.
struct BiasScan {
    struct Args {
        MaskSel ms;
        const float *coef, *g;  // [Q]
        const int32_t *boff;    // [Q]
        const float *bias;      // [n_bias][S]
        int *dom;               // [Q]
        int64_t fstride;
        uint32_t *F;
    };
    // one 16-byte entry per block query: the epilogue reads it with one LDS load
    struct alignas(16) Entry {
        float coef, g;
        int boff;  // fp32 entries from `bias` to the query's column, -1 = the zero column
        int moff;  // word offset of the query's mask, -1 = the empty mask (also: past Q), -2 = no mask
    };
    template <int QT>
    struct QState {
        Entry e[QT * 16];
    };
    struct View {};
    template <class QS>
    static __device__ __forceinline__ void load_query(QS &qs, const Args &a, int i, int q, bool live) {
        qs.e[i] = {live ? a.coef[q] : 0.f, live ? a.g[q] : 0.f, live ? a.boff[q] : -1,
                   !live ? -1 : (a.ms.words ? (int)mask_offset(a.ms, q) : -2)};
    }
    static __device__ __forceinline__ View view(const Args &, const RingView &) { return {}; }
    // the 16 selection bits of `tile` for the mask at word offset off, the slots at and past n cleared; what depends on
    // the tile alone is scalar (MaskScan::tile_bits)
    static __device__ __forceinline__ uint32_t tile_bits(const Args &a, int off, const TileLane &l) {
        if (off == -1) return 0u;
        const int tile = __builtin_amdgcn_readfirstlane((int)l.tile);
        const int64_t left = l.n - (int64_t)tile * 16;  // >= 1: the scan visits tiles that hold a live slot
        const uint32_t live = left < 16 ? (1u << left) - 1u : 0xffffu;
        if (off < 0) return live;
        // a 32-bit byte offset from the masks' base (the host refuses more than 2^30 words of masks): one address VGPR
        const uint32_t byte = (uint32_t)off * 4u + (uint32_t)tile * 2u;
        return *reinterpret_cast<const uint16_t *>(reinterpret_cast<const char *>(a.ms.words) + byte) & live;
    }
    template <int QT>
    static __device__ __forceinline__ bool skip_tile(const QState<QT> &qs, const Args &a, const TileLane &l) {
        if (!a.ms.words) return false;  // uniform: a kernel argument
        // lane i < QT * 16 reads the tile's bits of block query i; wave-uniform: some query selects some live row
        const uint32_t b = l.lane < QT * 16 ? tile_bits(a, qs.e[l.lane].moff, l) : 0u;
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
        // the lane's four slots inside a column, in fp32 entries: scalar tile + the lane's 4 h
        const uint32_t tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)l.tile);
        const uint32_t p32 = tile * 16u + 4u * (uint32_t)l.h;
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const int q = l.q0 + 16 * t + l.r16;
            if (q >= l.Q) continue;
            // The entry is the same for every tile, and the compiler knows it: it loads the entries before the tile loop,
            // and coef, g and boff of each query tile stay live across the MFMA loop next to the mask offset that MaskScan
            // keeps there too: 80 + 8 registers at QT = 2 against MaskScan's 72 + 8, 60 + 4 against 58 + 4 at QT = 1.
            // Keeping the load here (an index the compiler cannot see through) makes the epilogue the peak instead:
            // 82 + 8, and 78 + 8 with the query tiles fenced apart.
            const Entry en = qs.e[16 * t + l.r16];
            const uint32_t bits = tile_bits(a, en.moff, l) >> (4 * l.h);  // the lane's four slots
            const int bo = en.boff;
            // one 16-byte load at a 32-bit byte offset from the bias base (below 2^30 values: the offset fits); slots
            // p0 .. p0 + 3 are below S, the columns being padded to 64 rows
            float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (bo >= 0)
                bv = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(a.bias) + ((uint32_t)bo + p32) * 4u);
            const float b4[4] = {bv.x, bv.y, bv.z, bv.w};
            const float cf = en.coef, gq = en.g;
            uint32_t key[4];
            bool wide = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool sel = (bits >> j) & 1u;
                const float B = __fadd_rn(__fmul_rn(cf, s[t][j]), __fmul_rn(gq, b4[j]));
                key[j] = sel ? okey32(B) : 0u;
                wide |= sel && !(fabsf(b4[j]) <= BIAS_B_MAX);
            }
            if (wide) atomicOr(a.dom + q, 1);  // rare: a selected row's bias outside the bound's domain
            *reinterpret_cast<uint4 *>(a.F + (size_t)q * a.fstride + l.p0()) = make_uint4(key[0], key[1], key[2], key[3]);
        }
    }
};

// ---- finalize ----------------------------------------------------------------------------------------------
// One block per query; dynamic LDS: the query.  Ranks the C candidates by (fp32 key desc, order asc): the first
// nc = min(C, M) get their exact S, the (M+1)-th (if any) bounds every other selected row.
template <int DT>
__global__ void __launch_bounds__(BIAS_THREADS)
    bias_finalize_kernel(const uint16_t *__restrict__ mem, const double *__restrict__ norm64,
                         const uint16_t *__restrict__ queries, const double *__restrict__ weights,
                         const float *__restrict__ bias, const double *__restrict__ qn_all,
                         const int32_t *__restrict__ boff, const int *__restrict__ dom,
                         const int64_t *__restrict__ d_total, int64_t cap, int ring, int D,
                         const int *__restrict__ cand_o, const uint32_t *__restrict__ cand_k,
                         const int *__restrict__ cand_n, int M, int k, int use_min, double min_score, int64_t row_stride,
                         int64_t row_offset, double *__restrict__ out_scores, int64_t *__restrict__ out_rows,
                         int *__restrict__ uncertified, int *__restrict__ flags, int *__restrict__ user_flags) {
    extern __shared__ __attribute__((aligned(16))) char bf_dyn[];
    uint16_t *ql = reinterpret_cast<uint16_t *>(bf_dyn);  // [D]
    __shared__ int so[SCMAX], lo_[SCMAX];
    __shared__ uint32_t sk[SCMAX], lk[SCMAX];
    __shared__ double es[SCMAX];
    __shared__ int flag_sh;
    const int q = blockIdx.x, tid = threadIdx.x;
    const RingView rv = ring_view(*d_total, cap, ring);
    const int C = cand_n[q];
    if (C < 0) {  // uniform: more rows at the cut than the buffer holds -> the exhaustive redo answers this query
        for (int i = tid; i < k; i += BIAS_THREADS) {
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
    for (int i = tid; i < D / 8; i += BIAS_THREADS)
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
    __syncthreads();
    const double qn = qn_all[q];
    const double beta = weights ? weights[q] : 1.0;
    const int bo = boff[q];
    if (tid < nc) {
        const int64_t p = slot_of(rv, so[tid]);
        const double e = ref_cosine(ref_dot<DT>(ql, mem + (size_t)p * D, D), qn, norm64[p]);
        es[tid] = bias_exact(e, beta, bo >= 0 ? bias[(size_t)bo + p] : 0.f);
    }
    __syncthreads();
    if (tid < nc) {
        const double e = es[tid];
        const int o = so[tid];
        int r = 0;
        for (int d = 0; d < nc; ++d) r += (es[d] > e || (es[d] == e && so[d] < o)) ? 1 : 0;
        if (r < k) {
            const bool pass = passes_min(use_min, e, min_score);
            out_scores[(size_t)q * k + r] = pass ? e : 0.0;
            out_rows[(size_t)q * k + r] = pass ? (rv.base + o) * row_stride + row_offset : -1;
        }
        // certification: the exact k-th S against the best scanned score of a selected row that was not re-scored
        const int kth = (k < nc ? k : nc) - 1;
        if (r == kth && C > M) {
            const double Bs = (double)dekey32(sk[M]);
            if (!(e > __dadd_rn(Bs, eps_bias(D, Bs)))) flag_sh = VM_FLAG_GAP;
        }
    }
    for (int i = nc + tid; i < k; i += BIAS_THREADS) {
        out_scores[(size_t)q * k + i] = 0.0;
        out_rows[(size_t)q * k + i] = -1;
    }
    __syncthreads();
    if (tid == 0) {
        int f = flag_sh;
        // domain of the bound: the weight or the query's norm (pack), a selected row's bias (scan), or a stored bf16 row's
        // norm
        if (f == VM_FLAG_CERTIFIED && rv.n > 0) {
            bool outside = dom[q] != 0;
            if constexpr (DT == VM_BF16) outside |= d_total[VM_GSTATE_OUTSIDE] != 0;
            if (outside) f = VM_FLAG_GAP;
        }
        flags[q] = f;
        if (user_flags) user_flags[q] = f;
        if (f && uncertified) atomicAdd(uncertified, 1);
    }
}

// ---- redo ----------------------------------------------------------------------------------------------------
constexpr int BIAS_CHUNK = VM_REDO_CHUNK_SCOPED;

// topk_redo_scan_kernel's structure (topk_exact.hip) with the biased score: grid = nblk row blocks; every block walks all
// Q flags and, for each flagged query, scores its slice of age orders exactly - the rows pred admits - and keeps the
// slice's stable top-k: part[(block * Q + q) * k + i] = {S fp64, age order int64}.  Dynamic LDS: the query.
template <int DT, class P>
__global__ void __launch_bounds__(BIAS_THREADS)
    bias_redo_scan_kernel(const uint16_t *__restrict__ queries, const double *__restrict__ weights,
                          const float *__restrict__ bias, const double *__restrict__ qn_all,
                          const int32_t *__restrict__ boff, const uint16_t *__restrict__ rows,
                          const double *__restrict__ norm64, const int64_t *__restrict__ d_total, int64_t cap, int ring,
                          int D, int Q, int k, const int32_t *__restrict__ flags, double *__restrict__ part_s,
                          int64_t *__restrict__ part_o, const P pred) {
    constexpr bool SCOPED = P::scoped;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint16_t *ql = reinterpret_cast<uint16_t *>(smem);  // [D]
    __shared__ double sc[BIAS_CHUNK];
    __shared__ uint8_t live[BIAS_CHUNK];
    __shared__ double run_s[SKMAX], new_s[SKMAX], red_s[BIAS_THREADS / 64];
    __shared__ int64_t run_o[SKMAX], new_o[SKMAX], red_o[BIAS_THREADS / 64];
    const int tid = threadIdx.x;
    const RingView rv = ring_view(*d_total, cap, ring);
    const int64_t per = (rv.n + gridDim.x - 1) / gridDim.x;
    const int64_t lo = (int64_t)blockIdx.x * per;
    const int64_t hi = lo + per < rv.n ? lo + per : rv.n;
    int any = 0;  // the common launch has no flagged query at all
    for (int i = tid; i < Q; i += BIAS_THREADS) any |= flags[i];
    if (!__syncthreads_or(any)) return;
    for (int q = 0; q < Q; ++q) {
        if (flags[q] == 0) continue;  // uniform
        __syncthreads();
        for (int i = tid; i < D / 8; i += BIAS_THREADS)
            reinterpret_cast<uint4 *>(ql)[i] = reinterpret_cast<const uint4 *>(queries + (size_t)q * D)[i];
        if (tid < k) {
            run_s[tid] = -INFINITY;
            run_o[tid] = -1;
        }
        __syncthreads();
        const double qn = qn_all[q];
        const double beta = weights ? weights[q] : 1.0;
        const int bo = boff[q];
        const typename P::Q pq = pred.at(q);
        for (int64_t c0 = lo; c0 < hi; c0 += BIAS_CHUNK) {
            const int cn = (int)(hi - c0 < BIAS_CHUNK ? hi - c0 : BIAS_CHUNK);
            int mine = 0;
            for (int i = tid; i < cn; i += BIAS_THREADS) {
                const int64_t p = slot_of(rv, c0 + i);
                bool in = true;
                if constexpr (SCOPED) in = pq.in(p);
                live[i] = in ? 1 : 0;
                if (in) {
                    const double e = ref_cosine(ref_dot<DT>(ql, rows + (size_t)p * D, D), qn, norm64[p]);
                    sc[i] = bias_exact(e, beta, bo >= 0 ? bias[(size_t)bo + p] : 0.f);
                    mine = 1;
                }
            }
            if (!__syncthreads_or(mine)) continue;  // uniform: nothing of this chunk is admitted
            // candidates = this chunk's scores followed by the running list
            block_select<BIAS_THREADS>(cn + k, k,
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
            part_s[((size_t)blockIdx.x * Q + q) * k + tid] = run_s[tid];
            part_o[((size_t)blockIdx.x * Q + q) * k + tid] = run_o[tid];
        }
    }
}

// ---- builders ----------------------------------------------------------------------------------------------
// Thread = one entry of row_ids: values[i] goes to the slot of a live row.  -1, an id that is not row * stride + offset,
// and a row that is not live are skipped (mask_from_rows_kernel's rules).  Two entries that name one row race: one of their
// values stays.
__global__ void __launch_bounds__(256)
    bias_from_rows_kernel(const int64_t *__restrict__ row_ids, const float *__restrict__ values, int64_t n,
                          int64_t row_stride, int64_t row_offset, const int64_t *__restrict__ d_total, int64_t cap,
                          int ring, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t id = row_ids[i];
    if (id < 0) return;
    const int64_t d = id - row_offset;
    if (d < 0 || d % row_stride != 0) return;
    const int64_t r = d / row_stride;
    const RingView rv = ring_view(*d_total, cap, ring);
    if (r < rv.base || r >= rv.base + rv.n) return;
    out[r % cap] = values[i];  // = slot_of(rv, r - rv.base): below S
}

// Thread = one slot; the grid covers all S slots, so every entry is written.  Linear recency: a live slot with tag
// t != INT64_MIN gets fl32(per_ms * ((t & (2^40 - 1)) - t_ref_ms)), the difference exact in int64 and in fp64; an untagged
// live row and a slot without a live row get `fill`.
__global__ void __launch_bounds__(256)
    bias_from_tags_kernel(const int64_t *__restrict__ tag, int64_t t_ref_ms, double per_ms, float fill,
                          const int64_t *__restrict__ d_total, int64_t cap, int ring, int64_t S, float *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= S) return;
    const int64_t n = ring_view(*d_total, cap, ring).n;
    float v = fill;
    if (p < n) {
        const int64_t tg = tag[p];
        if (tg != INT64_MIN) {
            const int64_t d = (tg & (((int64_t)1 << 40) - 1)) - t_ref_ms;
            v = (float)__dmul_rn(per_ms, (double)d);
        }
    }
    out[p] = v;
}

// ---- host --------------------------------------------------------------------------------------------------
// vm_key_image_plan for Q key rows, then what the pack leaves
struct BPlan : SPlan {
    size_t off_qn, off_coef, off_g, off_boff, off_dom, bias_total;
};

BPlan bias_plan(const vm_memory *m, int Q, int k) {
    BPlan p;
    static_cast<SPlan &>(p) = vm_key_image_plan(m, Q, k);
    WsBump ws;
    ws.off = p.total;
    p.off_qn = ws.take((size_t)Q * 8);
    p.off_coef = ws.take((size_t)Q * 4);
    p.off_g = ws.take((size_t)Q * 4);
    p.off_boff = ws.take((size_t)Q * 4);
    p.off_dom = ws.take((size_t)Q * 4);
    p.bias_total = ws.off;
    return p;
}

// RowCall (score_mode raw) and what a biased call adds to it
struct BiasCall : RowCall {
    const float *bias;
    int n_bias;
    const int32_t *bias_index;
    const double *weights;  // null: 1.0 for every query
    const uint32_t *masks;  // null: every live row
    int n_masks;
    const int32_t *mask_index;
    size_t ws_bytes;
};

int bias_check(vm_memory *m, const BiasCall &c, const char *who) {
    vm_ctx *ctx = m->ctx;
    if (c.k < 1 || c.k > SKMAX) return vm_fail(ctx, VM_ERR_INVALID, "%s: k=%d outside [1, %d]", who, c.k, SKMAX);
    if (c.Q < 1 || c.Q > BIAS_Q_MAX) return vm_fail(ctx, VM_ERR_INVALID, "%s: Q=%d outside [1, %d]", who, c.Q, BIAS_Q_MAX);
    if (!c.queries || !c.bias) return vm_fail(ctx, VM_ERR_INVALID, "%s: null queries or bias", who);
    if (!c.out_scores || !c.out_rows) return vm_fail(ctx, VM_ERR_INVALID, "%s: null outputs", who);
    if (c.row_stride < 1) return vm_fail(ctx, VM_ERR_INVALID, "%s: row_stride=%lld < 1", who, (long long)c.row_stride);
    if ((uintptr_t)c.bias & 15) return vm_fail(ctx, VM_ERR_INVALID, "%s: bias must be 16-byte aligned", who);
    if (c.n_bias < 1 || !(c.bias_index || c.n_bias == 1 || c.n_bias == c.Q))
        return vm_fail(ctx, VM_ERR_INVALID, "%s: %d bias columns for %d queries need a bias_index", who, c.n_bias, c.Q);
    if ((int64_t)c.n_bias * bias_stride(m) > ((int64_t)1 << 30))
        return vm_fail(ctx, VM_ERR_UNSUPPORTED, "%s: more than 2^30 bias values", who);
    if (c.masks)
        if (int rc = mask_operand_check(m, c.masks, c.n_masks, c.mask_index, c.Q, who)) return rc;
    const size_t need = bias_plan(m, c.Q, c.k).bias_total;
    if (!c.ws || c.ws_bytes < need) return vm_fail(ctx, VM_ERR_INVALID, "%s: workspace %zu < %zu", who, c.ws_bytes, need);
    if (((uintptr_t)c.ws & 255) || ((uintptr_t)c.queries & 15) || ((uintptr_t)c.weights & 7))
        return vm_fail(ctx, VM_ERR_INVALID, "%s: workspace must be 256-byte, queries 16-byte and weights 8-byte aligned",
                       who);
    return VM_OK;
}

// what both entries need of the workspace
struct BiasBufs {
    double *qn;
    float *coef, *g;
    int32_t *boff;
    int *dom, *flags;
};
BiasBufs bias_bufs(const BPlan &p, char *ws) {
    return {(double *)(ws + p.off_qn),    (float *)(ws + p.off_coef), (float *)(ws + p.off_g),
            (int32_t *)(ws + p.off_boff), (int *)(ws + p.off_dom),    (int *)(ws + p.off_flags)};
}

template <int DT>
int bias_pack(vm_memory *m, const BiasCall &c, const BiasBufs &b) {
    bias_pack_kernel<DT><<<c.Q, 64, (size_t)m->D * 2, c.stream>>>((const uint16_t *)c.queries, c.weights, c.bias_index,
                                                             c.n_bias, bias_stride(m), c.Q, m->D, b.qn, b.coef, b.g,
                                                             b.boff, b.dom);
    VM_LAUNCH_CHECK(m->ctx);
    return VM_OK;
}

template <int DT, class P>
int bias_redo(vm_memory *m, const BPlan &p, const BiasCall &c, const BiasBufs &b, const P &pred) {
    vm_prof_scope prof(m->ctx, VM_PROF_TOPK_EXACT, c.stream);
    double *part_s = (double *)(c.ws + p.off_ps);
    int64_t *part_o = (int64_t *)(c.ws + p.off_po);
    bias_redo_scan_kernel<DT, P><<<p.nblk, BIAS_THREADS, (size_t)m->D * 2, c.stream>>>(
        (const uint16_t *)c.queries, c.weights, c.bias, b.qn, b.boff, m->rows, m->norm64, m->d_total, m->cap, m->ring,
        m->D, c.Q, c.k, b.flags, part_s, part_o, pred);
    VM_LAUNCH_CHECK(m->ctx);
    return vm_topk_redo_merge(m, part_s, part_o, p.nblk, c.Q, c.k, b.flags, c.use_min, c.min_score, VM_SCORE_RAW,
                              c.row_stride, c.row_offset, c.out_scores, c.out_rows, nullptr, nullptr, c.stream);
}

// pack -> scan -> cut -> compact -> select -> finalize -> redo, or (exact) pack -> every query flagged -> redo
template <int DT>
int bias_run(vm_memory *m, const BiasCall &c, bool exact) {
    vm_ctx *ctx = m->ctx;
    hipStream_t st = c.stream;
    char *ws = c.ws;
    const BPlan p = bias_plan(m, c.Q, c.k);
    const BiasBufs b = bias_bufs(p, ws);
    const MaskSel ms = {c.masks, c.mask_index, c.n_masks, mask_words(m)};
    if (!exact) {
        uint32_t *F = (uint32_t *)ws;
        {
            vm_prof_scope prof(ctx, VM_PROF_TOPK_SCAN, st);
            if (int rc = bias_pack<DT>(m, c, b)) return rc;
            const BiasScan::Args a = {ms, b.coef, b.g, b.boff, c.bias, b.dom, p.fstride, F};
            if (int rc = vm_tile_scan<DT, BiasScan>(m, p, c.queries, c.Q, a, st)) return rc;
        }
        {
            vm_prof_scope prof(ctx, VM_PROF_TOPK_FINALIZE, st);
            if (int rc = vm_key_image_select(m, p, F, c.Q, ws, st)) return rc;
            bias_finalize_kernel<DT><<<c.Q, BIAS_THREADS, (size_t)m->D * 2, st>>>(
                m->rows, m->norm64, (const uint16_t *)c.queries, c.weights, c.bias, b.qn, b.boff, b.dom, m->d_total, m->cap,
                m->ring, m->D, (const int *)(ws + p.off_co), (const uint32_t *)(ws + p.off_ck),
                (const int *)(ws + p.off_cn), p.M, c.k, c.use_min, c.min_score, c.row_stride, c.row_offset, c.out_scores,
                c.out_rows, c.out_uncertified, b.flags, c.out_query_flags);
            VM_LAUNCH_CHECK(ctx);
        }
    } else {
        if (int rc = bias_pack<DT>(m, c, b)) return rc;
        if (int rc = vm_fill_flags(m, b.flags, c.Q, st)) return rc;
    }
    if (c.masks) return bias_redo<DT>(m, p, c, b, MaskScope{ms});
    return bias_redo<DT>(m, p, c, b, NoScope{});
}

int bias_entry(vm_memory *m, const BiasCall &c, bool exact, const char *who) {
    if (!m) return VM_ERR_INVALID;
    if (int rc = bias_check(m, c, who)) return rc;
    return vm_by_dtype(m, [&](auto dt) { return bias_run<decltype(dt)::value>(m, c, exact); });
}

}  // namespace

extern "C" int64_t vm_memory_bias_stride(const vm_memory *m) { return m ? bias_stride(m) : 0; }

extern "C" size_t vm_topk_bias_workspace_bytes(const vm_memory *m, int Q, int k) {
    if (!m || Q < 1 || Q > BIAS_Q_MAX || k < 1 || k > SKMAX) return 0;
    return bias_plan(m, Q, k).bias_total;
}

extern "C" int vm_topk_cosine_biased(vm_memory *m, const void *queries, int Q, int k, const float *bias, int n_bias,
                                     const int32_t *bias_index, const double *bias_weight, const uint32_t *masks,
                                     int n_masks, const int32_t *mask_index, int use_min_score, double min_score,
                                     int64_t row_stride, int64_t row_offset, double *out_scores, int64_t *out_rows,
                                     int32_t *out_uncertified, int32_t *out_query_flags, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    const BiasCall c = {{queries, Q, k, use_min_score, min_score, VM_SCORE_RAW, row_stride, row_offset, out_scores,
                         out_rows, out_uncertified, out_query_flags, (char *)workspace, (hipStream_t)stream},
                        bias, n_bias, bias_index, bias_weight, masks, n_masks, mask_index, workspace_bytes};
    return bias_entry(m, c, false, "vm_topk_cosine_biased");
}

extern "C" int vm_topk_cosine_biased_exact(vm_memory *m, const void *queries, int Q, int k, const float *bias,
                                           int n_bias, const int32_t *bias_index, const double *bias_weight,
                                           const uint32_t *masks, int n_masks, const int32_t *mask_index,
                                           int use_min_score, double min_score, int64_t row_stride, int64_t row_offset,
                                           double *out_scores, int64_t *out_rows, void *workspace,
                                           size_t workspace_bytes, void *stream) {
    const BiasCall c = {{queries, Q, k, use_min_score, min_score, VM_SCORE_RAW, row_stride, row_offset, out_scores,
                         out_rows, nullptr, nullptr, (char *)workspace, (hipStream_t)stream},
                        bias, n_bias, bias_index, bias_weight, masks, n_masks, mask_index, workspace_bytes};
    return bias_entry(m, c, true, "vm_topk_cosine_biased_exact");
}

extern "C" int vm_bias_from_rows(vm_memory *m, const int64_t *row_ids, const float *values, int64_t n,
                                 int64_t row_stride, int64_t row_offset, int clear_first, float *out_bias,
                                 void *stream) {
    if (!m) return VM_ERR_INVALID;
    vm_ctx *ctx = m->ctx;
    if (!out_bias || ((uintptr_t)out_bias & 15) || n < 0 || (n > 0 && (!row_ids || !values)) || row_stride < 1)
        return vm_fail(ctx, VM_ERR_INVALID, "vm_bias_from_rows: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (clear_first) VM_HIP(ctx, hipMemsetAsync(out_bias, 0, (size_t)bias_stride(m) * 4, st));
    if (n == 0) return VM_OK;
    bias_from_rows_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(row_ids, values, n, row_stride, row_offset,
                                                                     m->d_total, m->cap, m->ring, out_bias);
    VM_LAUNCH_CHECK(ctx);
    return VM_OK;
}

extern "C" int vm_bias_from_tags(vm_memory *m, int64_t t_ref_ms, double per_ms, float fill, float *out_bias,
                                 void *stream) {
    if (!m) return VM_ERR_INVALID;
    vm_ctx *ctx = m->ctx;
    if (!m->tag) return vm_fail(ctx, VM_ERR_INVALID, "vm_bias_from_tags: the memory is not tagged");
    if (!out_bias || ((uintptr_t)out_bias & 15)) return vm_fail(ctx, VM_ERR_INVALID, "vm_bias_from_tags: bad arguments");
    const int64_t S = bias_stride(m);
    bias_from_tags_kernel<<<(unsigned)((S + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        m->tag, t_ref_ms, per_ms, fill, m->d_total, m->cap, m->ring, S, out_bias);
    VM_LAUNCH_CHECK(ctx);
    return VM_OK;
}
