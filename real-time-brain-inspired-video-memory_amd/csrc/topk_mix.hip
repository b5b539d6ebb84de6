// Mixed-query cosine top-k: the k best rows by a WEIGHTED SUM OF COSINES (include/vidmem.h vm_topk_cosine_mix).  A mixed
// query is up to 16 term vectors with one fp64 weight each - text plus picture, Rocchio feedback with negative terms, the
// mean of a few examples - and W(c, r) = sum_j w[c][j] * e_j(r), e_j = the reference cosine of term j and row r, summed
// left to right from 0.0 with one rounding per product and per addition.
//
// The masked search (topk_mask.hip) with another score, and built from the same parts:
//   pack     : the terms of query c become one zero-padded 16-column query tile [16][D]; per term the fp32 coefficient
//              fl32(w_j / ||q_j||) and the fp64 norm, per query A = sum |w_j| and the flag of the bound's domain
//   scan     : topk_tile_scan.h under the MixScan policy below, launched with 16 C columns: ONE TILE IS ONE QUERY.  The
//              sixteen MFMA columns that a one-vector query leaves empty hold the terms; the epilogue scales each
//              column by its coefficient and sums the 16 lanes that hold one row's 16 scores, so only one key column per
//              mixed query reaches memory: F[c][slot] = okey32(B) for a selected live row, 0 for any other
//   select   : topk_key_image.hip's vm_key_image_select, with Q = C
//   finalize : mix_finalize_kernel: the exact W of the best M candidates; certified when at most M rows are selected
//              or the exact k-th W clears dekey32(key of the (M+1)-th) + eps_mix(D, A), strictly
//   redo     : mix_redo_scan_kernel (topk_redo_scan_kernel's structure, every admitted row scored exactly), then
//              vm_topk_redo_merge as it is
// Every launch reads the row count from the device and sizes its grid from the capacity: capturable.
//
// The any/all search (vm_topk_cosine_fold) is the same route with another reduction over the terms: the
// MAXIMUM or the MINIMUM of the weighted cosines, F(c, r) = max_j / min_j fl64(w_j * e_j(r)) by a strict compare taken
// j = 0 .. J-1, T(c, r) = the first term that attains it.  Every kernel here takes the reduction as the template
// parameter OP (MIX_OP_SUM, VM_FOLD_MAX, VM_FOLD_MIN); the sum instantiations are the mixed search's kernels as they were.
// What differs: the pack's magnitude A is max |w_j|, not the sum; the scan policy FoldScan keeps the padding columns
// J .. 15 out of the reduction (a zero column must not vote) and reduces with max / min, which is exact, so the bound
// eps_fold = A (cert_eps(D) + 2^-21) needs A = max |w_j| only; a zero weight is NOT neutral (its product +-0.0 takes
// part); and one small kernel after either path writes T of the returned rows (fold_terms_kernel).
#include "topk_scope_select.h"
#include "topk_tile_scan.h"

namespace {

constexpr int MIX_OP_SUM = 2;      // the template parameter OP: the sum, or a vm_fold_op; never a caller's value
constexpr int MIX_J = 16;          // terms per mixed query = columns of one query tile
constexpr int MIX_THREADS = 256;   // pack, finalize, redo
constexpr double MIX_W_MIN = 9.5367431640625e-07;  // 2^-20: the weight domain of the bound, |w| in [2^-20, 2^20] or 0
constexpr double MIX_W_MAX = 1048576.0;            // 2^20

// The bound of the scanned score B against the exact W inside the domain: each fp32 column score times
// 1/||q_j|| lies within cert_eps(D) of e_j; the coefficient's rounding, the product's and four levels of fp32 addition
// cost at most 2^-24 relative each on magnitudes bounded by A (1 + small): 6 roundings, 2^-21 with slack.
__device__ __forceinline__ double eps_mix(int D, double A) {
    return __dmul_rn(A, __dadd_rn(cert_eps(D), 4.76837158203125e-07));
}
// The fold's bound is the same expression with A = max |w_j|: column j's scaled score lies within
// |w_j| (cert_eps(D) + 2^-23 (1 + small)) of w_j e_j - the coefficient's rounding and the product's, 2^-24 relative each on
// a magnitude of at most |w_j| (1 + cert_eps) -, and max and min move by no more than their most-moved argument and round
// nothing.  2^-21 leaves a factor of four over the two roundings.
__device__ __forceinline__ double eps_fold(int D, double A) { return eps_mix(D, A); }

// The fold over the J products w_j * e_j: a strict compare taken left to right, so the first term wins a tie and a zero
// of one sign is never replaced by the other.  e(j): the exact cosine of term j, from LDS (finalize, the winning term) or
// computed as the loop goes (redo).  -> F, and T in arg.  The one statement of the defining compare.
template <int OP, class E>
__device__ __forceinline__ double fold_terms(const double *w, E e, int J, int &arg) {
    double acc = __dmul_rn(w[0], e(0));
    arg = 0;
    for (int j = 1; j < J; ++j) {
        const double p = __dmul_rn(w[j], e(j));
        if (OP == VM_FOLD_MAX ? p > acc : p < acc) {
            acc = p;
            arg = j;
        }
    }
    return acc;
}

// ---- pack --------------------------------------------------------------------------------------------------
// One block per mixed query.  tiles [C][16][D]: the J terms, then zero columns.  coef / qn [C][16], A / dom [C].
// A: the sum of the |w_j| (the mixed search), their maximum (a fold).
template <int DT, int OP>
__global__ void __launch_bounds__(MIX_THREADS)
    mix_pack_kernel(const uint16_t *__restrict__ terms, const double *__restrict__ weights, int J, int D,
                    uint16_t *__restrict__ tiles, float *__restrict__ coef, double *__restrict__ qn,
                    double *__restrict__ A, int *__restrict__ dom) {
    __shared__ double aw[MIX_J];
    __shared__ int bad[MIX_J];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int chunks = D / 8;
    const uint4 *src = reinterpret_cast<const uint4 *>(terms + (size_t)c * J * D);
    uint4 *dst = reinterpret_cast<uint4 *>(tiles + (size_t)c * MIX_J * D);
    for (int i = tid; i < MIX_J * chunks; i += MIX_THREADS) dst[i] = i < J * chunks ? src[i] : make_uint4(0, 0, 0, 0);
    if (tid < MIX_J) {
        double w = 0.0, nrm = 0.0;
        if (tid < J) {
            w = weights[(size_t)c * J + tid];
            nrm = __dsqrt_rn(ref_sumsq<DT>(terms + ((size_t)c * J + tid) * D, D));
        }
        const double a = fabs(w);
        coef[c * MIX_J + tid] = (w == 0.0 || nrm == 0.0) ? 0.f : (float)__ddiv_rn(w, nrm);
        qn[c * MIX_J + tid] = nrm;
        aw[tid] = a;
        bad[tid] = ((a != 0.0 && !(a >= MIX_W_MIN && a <= MIX_W_MAX)) || cert_norm_outside(nrm)) ? 1 : 0;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        int b = 0;
        for (int j = 0; j < MIX_J; ++j) {
            if constexpr (OP == MIX_OP_SUM) s = __dadd_rn(s, aw[j]);
            else s = aw[j] > s ? aw[j] : s;  // the padding entries are 0.0
            b |= bad[j];
        }
        A[c] = s;
        dom[c] = b;
    }
}

// ---- scan --------------------------------------------------------------------------------------------------
// x of the lane R places away in its row of 16 lanes, cyclically (DPP row_ror; every lane of a wave is active where the
// scan's epilogue runs: the tile loop, the skip and the test for a tile past Q are wave-uniform)
template <int R>
__device__ __forceinline__ float row_ror(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x120 + R, 0xf, 0xf, false));
}

// The mixed policy of the tile scan.  The scan's "queries" are the 16 C columns of the packed tiles, so query tile t of a
// block is mixed query q0 / 16 + t, and F has one key row per MIXED query: F[c * fstride + slot] = the order-preserving
// key of B = sum over the 16 columns of coef * score, or 0 when c's mask does not select the slot or the slot is past
// the live rows.  ms.words == nullptr: no mask, every live row is selected.
struct MixScan {
    struct Args {
        MaskSel ms;
        const float *coef;  // [C][16]
        int64_t fstride;
        uint32_t *F;
    };
    template <int QT>
    struct QState {
        float coef[QT * 16];
    };
    struct View {};
    template <class QS>
    static __device__ __forceinline__ void load_query(QS &qs, const Args &a, int i, int q, bool live) {
        qs.coef[i] = live ? a.coef[q] : 0.f;
    }
    // Word offset of the mask of the block's mixed query t: -1 = the empty mask (also: the tile is past Q), -2 = no mask.
    // One mask per 16 columns, and q0 comes from the block index: the offset is scalar, read through the constant address
    // space (no kernel writes a mask or an index; TagScope::at, vm_internal.h), and needs no place in the LDS state - from
    // there it came back as a VGPR that stayed live across the MFMA loop.
    static __device__ __forceinline__ int tile_off(const Args &a, const TileLane &l, int t) {
        typedef const __attribute__((address_space(4))) int32_t *scalar_ptr;
        const int c = l.q0 / 16 + t;
        if (16 * c >= l.Q) return -1;
        if (!a.ms.words) return -2;
        const int64_t i = a.ms.index ? ((scalar_ptr)a.ms.index)[c] : (a.ms.n_masks == 1 ? 0 : c);
        return i < 0 || i >= a.ms.n_masks ? -1 : (int)(i * a.ms.W);  // below 2^30: the host refuses more words of masks
    }
    static __device__ __forceinline__ View view(const Args &, const RingView &) { return {}; }
    // The 16 selection bits of `tile` for the mask at word offset off (tile_off), the slots at and past n cleared.  All of
    // it is the same in every lane: off is scalar, the tile comes through readfirstlane (MaskScan::tile_bits) and the mask
    // word is read through the constant address space, so the bits are one scalar load and nothing of them stays in VGPRs
    // across the MFMA loop.  Halfword tile & 1 of word tile >> 1, little endian.
    static __device__ __forceinline__ uint32_t tile_bits(const Args &a, int off, const TileLane &l) {
        typedef const __attribute__((address_space(4))) uint32_t *scalar_ptr;
        if (off == -1) return 0u;
        const int tile = __builtin_amdgcn_readfirstlane((int)l.tile);
        const int64_t left = l.n - (int64_t)tile * 16;  // >= 1: the scan visits tiles that hold a live slot
        const uint32_t live = left < 16 ? (1u << left) - 1u : 0xffffu;
        if (off < 0) return live;
        // the host refuses more than 2^30 words of masks: the word index fits an int
        return (((scalar_ptr)a.ms.words)[off + (tile >> 1)] >> ((tile & 1) * 16)) & live;
    }
    // The lane's four keys of the block's mixed query t: F[(q0 / 16 + t) * fstride + p0 ..].  The address is a scalar base
    // (the query's key row and the tile) plus the lane's 32-bit offset 4 h.  The base goes through readfirstlane, or the
    // compiler re-associates the sum into a loop-invariant 64-bit VGPR base per query tile (F + the key row + 4 h) plus the
    // tile, which stays live across the MFMA loop: 84 VGPRs at QT = 2 instead of 80.  The integer is turned back into a
    // GLOBAL pointer: as a generic one the store would be a flat one.
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ void store_keys(const Args &a, const TileLane &l, int t, u32x4 keys) {
        typedef __attribute__((address_space(1))) u32x4 *global_ptr;
        const int tile = __builtin_amdgcn_readfirstlane((int)l.tile);
        const uint64_t row = (uint64_t)(a.F + (size_t)(l.q0 / 16 + t) * a.fstride + (size_t)tile * 16);
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)row);
        const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(row >> 32));
        *(global_ptr)((((uint64_t)hi << 32) | lo) + (uint32_t)(16 * l.h)) = keys;
    }
    template <int QT>
    static __device__ __forceinline__ bool skip_tile(const QState<QT> &qs, const Args &a, const TileLane &l) {
        if (!a.ms.words) return false;  // uniform: a kernel argument
        uint32_t b = 0u;  // scalar: some mixed query of the block selects a live row of the tile
#pragma unroll
        for (int t = 0; t < QT; ++t) b |= tile_bits(a, tile_off(a, l, t), l);
        if (b != 0u) return false;
        if (l.r16 == 0) {  // a skipped tile only zeroes its keys: four lanes, four keys each, per mixed query
#pragma unroll
            for (int t = 0; t < QT; ++t)
                if (l.q0 + 16 * t < l.Q)
                    store_keys(a, l, t, u32x4{0u, 0u, 0u, 0u});
        }
        return true;
    }
    template <int QT>
    static __device__ __forceinline__ void epilogue(const QState<QT> &qs, const Args &a, const View &,
                                                    const TileLane &l, const float (&s)[QT][4]) {
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            if (l.q0 + 16 * t >= l.Q) continue;  // uniform
            const float cf = qs.coef[16 * t + l.r16];
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = cf * s[t][j];
            // Sum over the 16 lanes that share h - one DPP row - by rotations of 8, 4, 2, 1 lanes: after the rotation by r
            // the values repeat with period r, and lanes i and i + r add the same two values (fp32 addition commutes), so
            // every lane ends with the same bits.  DPP, not __shfl_xor: the shuffle's four lane addresses would stay in
            // VGPRs across the MFMA loop
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] += row_ror<8>(v[j]);
                v[j] += row_ror<4>(v[j]);
                v[j] += row_ror<2>(v[j]);
                v[j] += row_ror<1>(v[j]);
            }
            if (l.r16 == 0) store_selected(a, l, t, v);
        }
    }
    // lane r16 == 0 of each h: the keys of the lane's four reduced scores, 0 where the mask does not select the slot
    static __device__ __forceinline__ void store_selected(const Args &a, const TileLane &l, int t, const float (&v)[4]) {
        const uint32_t b = tile_bits(a, tile_off(a, l, t), l) >> (4 * l.h);  // four slots
        uint32_t key[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) key[j] = ((b >> j) & 1u) ? okey32(v[j]) : 0u;
        store_keys(a, l, t, u32x4{key[0], key[1], key[2], key[3]});
    }
};

// The fold policy of the tile scan: MixScan's state, masks, skip and stores, with the maximum (VM_FOLD_MAX) or minimum
// (VM_FOLD_MIN) over the query's J columns in place of the sum.  J is a kernel argument: uniform.  The padding columns
// J .. 15 hold zero vectors and would score 0; they take the reduction's neutral element BEFORE it, so they never vote.
// max / min of two floats is exact and commutes: after the four rotations every lane of a row holds the same bits.
template <int OP>
struct FoldScan : MixScan {
    struct Args : MixScan::Args {
        int J;
    };
    // pad: what a column adds to its scaled score before the reduction - -0.0 for a term (x + -0.0 = x for every x, either
    // zero included), the neutral element for a padding column, whose scaled score is the exact 0 of a zero vector.
    // From LDS like the coefficient: as a select on r16 < J the same thing costs four VGPRs across the MFMA loop
    // (84 at QT = 2, a wave per SIMD less than the mixed scan's 80).
    template <int QT>
    struct QState : MixScan::QState<QT> {
        float pad[QT * 16];
    };
    template <class QS>
    static __device__ __forceinline__ void load_query(QS &qs, const Args &a, int i, int q, bool live) {
        MixScan::load_query(qs, a, i, q, live);
        qs.pad[i] = (i & 15) < a.J ? -0.f : (OP == VM_FOLD_MAX ? -INFINITY : INFINITY);
    }
    template <int QT>
    static __device__ __forceinline__ void epilogue(const QState<QT> &qs, const Args &a, const View &,
                                                    const TileLane &l, const float (&s)[QT][4]) {
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            if (l.q0 + 16 * t >= l.Q) continue;  // uniform
            const float cf = qs.coef[16 * t + l.r16], pad = qs.pad[16 * t + l.r16];
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = cf * s[t][j] + pad;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = fold2(v[j], row_ror<8>(v[j]));
                v[j] = fold2(v[j], row_ror<4>(v[j]));
                v[j] = fold2(v[j], row_ror<2>(v[j]));
                v[j] = fold2(v[j], row_ror<1>(v[j]));
            }
            if (l.r16 == 0) store_selected(a, l, t, v);
        }
    }
    static __device__ __forceinline__ float fold2(float x, float y) {
        return OP == VM_FOLD_MAX ? fmaxf(x, y) : fminf(x, y);
    }
};

// ---- the exact score -----------------------------------------------------------------------------------------
// W of the row in slot p for the J terms in tl [J][D] (LDS): sum from 0.0, left to right, one rounding per product and
// per addition.  A fold: F of that row, fold_terms with the cosines computed as it goes.
template <int DT, int OP>
__device__ __forceinline__ double mix_exact(const uint16_t *tl, const double *w, const double *qn, int J, int D,
                                            const uint16_t *row, double rown) {
    if constexpr (OP == MIX_OP_SUM) {
        double acc = 0.0;
        for (int j = 0; j < J; ++j)
            acc = __dadd_rn(acc, __dmul_rn(w[j], ref_cosine(ref_dot<DT>(tl + (size_t)j * D, row, D), qn[j], rown)));
        return acc;
    } else {
        int arg;
        return fold_terms<OP>(
            w, [&](int j) { return ref_cosine(ref_dot<DT>(tl + (size_t)j * D, row, D), qn[j], rown); }, J, arg);
    }
}

// ---- finalize ----------------------------------------------------------------------------------------------
// One block per mixed query; dynamic LDS: the J terms.  Ranks the C candidates by (fp32 key desc, order asc): the first
// nc = min(C, M) get their exact W - one (candidate, term) cosine per thread and step, then one left-to-right sum per
// candidate (a fold: one fold_terms) -, the (M+1)-th (if any) bounds every other selected row.  Asum: the pack's A.
template <int DT, int OP>
__global__ void __launch_bounds__(MIX_THREADS)
    mix_finalize_kernel(const uint16_t *__restrict__ mem, const double *__restrict__ norm64,
                        const uint16_t *__restrict__ tiles, const double *__restrict__ weights,
                        const double *__restrict__ qn, const double *__restrict__ Asum, const int *__restrict__ dom,
                        const int64_t *__restrict__ d_total, int64_t cap, int ring, int D, int J,
                        const int *__restrict__ cand_o, const uint32_t *__restrict__ cand_k,
                        const int *__restrict__ cand_n, int M, int k, int use_min, double min_score, int64_t row_stride,
                        int64_t row_offset, double *__restrict__ out_scores, int64_t *__restrict__ out_rows,
                        int *__restrict__ uncertified, int *__restrict__ flags, int *__restrict__ user_flags) {
    extern __shared__ __attribute__((aligned(16))) char mf_dyn[];
    uint16_t *tl = reinterpret_cast<uint16_t *>(mf_dyn);  // [J][D]
    __shared__ int so[SCMAX], lo_[SCMAX];
    __shared__ uint32_t sk[SCMAX], lk[SCMAX];
    __shared__ double es[SCMAX];
    __shared__ double ec[(SCMAX - 32) * MIX_J];  // [nc <= M <= 80][16] cosines
    __shared__ double wl[MIX_J], ql[MIX_J];
    __shared__ int flag_sh;
    const int q = blockIdx.x, tid = threadIdx.x;
    const RingView rv = ring_view(*d_total, cap, ring);
    const int C = cand_n[q];
    if (C < 0) {  // uniform: more rows at the cut than the buffer holds -> the exhaustive redo answers this query
        for (int i = tid; i < k; i += MIX_THREADS) {
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
    for (int i = tid; i < J * (D / 8); i += MIX_THREADS)
        reinterpret_cast<uint4 *>(tl)[i] = reinterpret_cast<const uint4 *>(tiles + (size_t)q * MIX_J * D)[i];
    if (tid < C) {
        lo_[tid] = cand_o[(size_t)q * SCMAX + tid];
        lk[tid] = cand_k[(size_t)q * SCMAX + tid];
    }
    if (tid >= MIX_THREADS - MIX_J) {
        const int j = tid - (MIX_THREADS - MIX_J);
        wl[j] = j < J ? weights[(size_t)q * J + j] : 0.0;
        ql[j] = qn[q * MIX_J + j];
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
    for (int i = tid; i < nc * J; i += MIX_THREADS) {  // (candidate, term) pairs
        const int cd = i / J, j = i - cd * J;
        const int64_t p = slot_of(rv, so[cd]);
        ec[cd * MIX_J + j] = ref_cosine(ref_dot<DT>(tl + (size_t)j * D, mem + (size_t)p * D, D), ql[j], norm64[p]);
    }
    __syncthreads();
    if (tid < nc) {
        if constexpr (OP == MIX_OP_SUM) {
            double acc = 0.0;
            for (int j = 0; j < J; ++j) acc = __dadd_rn(acc, __dmul_rn(wl[j], ec[tid * MIX_J + j]));
            es[tid] = acc;
        } else {
            int arg;
            es[tid] = fold_terms<OP>(wl, [&](int j) { return ec[tid * MIX_J + j]; }, J, arg);
        }
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
        // certification: the exact k-th W against the best scanned score of a selected row that was not re-scored
        const int kth = (k < nc ? k : nc) - 1;
        if (r == kth && C > M &&
            !(e > __dadd_rn((double)dekey32(sk[M]), OP == MIX_OP_SUM ? eps_mix(D, Asum[q]) : eps_fold(D, Asum[q]))))
            flag_sh = VM_FLAG_GAP;
    }
    for (int i = nc + tid; i < k; i += MIX_THREADS) {
        out_scores[(size_t)q * k + i] = 0.0;
        out_rows[(size_t)q * k + i] = -1;
    }
    __syncthreads();
    if (tid == 0) {
        int f = flag_sh;
        // domain of the bound: a weight or a term norm outside it (pack), or a stored bf16 row's norm
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
constexpr int MIX_CHUNK = VM_REDO_CHUNK_SCOPED;

// topk_redo_scan_kernel's structure (topk_exact.hip) with the mixed score: grid = nblk row blocks; every block walks all
// C flags and, for each flagged query, scores its slice of age orders exactly - the rows pred admits - and keeps the
// slice's stable top-k: part[(block * C + c) * k + i] = {W fp64, age order int64}.  Dynamic LDS: the J terms.
template <int DT, int OP, class P>
__global__ void __launch_bounds__(MIX_THREADS)
    mix_redo_scan_kernel(const uint16_t *__restrict__ tiles, const double *__restrict__ weights,
                         const double *__restrict__ qn, const uint16_t *__restrict__ rows,
                         const double *__restrict__ norm64, const int64_t *__restrict__ d_total, int64_t cap, int ring,
                         int D, int C, int J, int k, const int32_t *__restrict__ flags, double *__restrict__ part_s,
                         int64_t *__restrict__ part_o, const P pred) {
    constexpr bool SCOPED = P::scoped;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint16_t *tl = reinterpret_cast<uint16_t *>(smem);  // [J][D]
    __shared__ double sc[MIX_CHUNK];
    __shared__ uint8_t live[MIX_CHUNK];
    __shared__ double run_s[SKMAX], new_s[SKMAX], red_s[MIX_THREADS / 64];
    __shared__ int64_t run_o[SKMAX], new_o[SKMAX], red_o[MIX_THREADS / 64];
    __shared__ double wl[MIX_J], ql[MIX_J];
    const int tid = threadIdx.x;
    const RingView rv = ring_view(*d_total, cap, ring);
    const int64_t per = (rv.n + gridDim.x - 1) / gridDim.x;
    const int64_t lo = (int64_t)blockIdx.x * per;
    const int64_t hi = lo + per < rv.n ? lo + per : rv.n;
    int any = 0;  // the common launch has no flagged query at all
    for (int i = tid; i < C; i += MIX_THREADS) any |= flags[i];
    if (!__syncthreads_or(any)) return;
    for (int q = 0; q < C; ++q) {
        if (flags[q] == 0) continue;  // uniform
        __syncthreads();
        for (int i = tid; i < J * (D / 8); i += MIX_THREADS)
            reinterpret_cast<uint4 *>(tl)[i] = reinterpret_cast<const uint4 *>(tiles + (size_t)q * MIX_J * D)[i];
        if (tid < k) {
            run_s[tid] = -INFINITY;
            run_o[tid] = -1;
        }
        if (tid >= MIX_THREADS - MIX_J) {
            const int j = tid - (MIX_THREADS - MIX_J);
            wl[j] = j < J ? weights[(size_t)q * J + j] : 0.0;
            ql[j] = qn[q * MIX_J + j];
        }
        __syncthreads();
        const typename P::Q pq = pred.at(q);
        for (int64_t c0 = lo; c0 < hi; c0 += MIX_CHUNK) {
            const int cn = (int)(hi - c0 < MIX_CHUNK ? hi - c0 : MIX_CHUNK);
            int mine = 0;
            for (int i = tid; i < cn; i += MIX_THREADS) {
                const int64_t p = slot_of(rv, c0 + i);
                bool in = true;
                if constexpr (SCOPED) in = pq.in(p);
                live[i] = in ? 1 : 0;
                if (in) {
                    sc[i] = mix_exact<DT, OP>(tl, wl, ql, J, D, rows + (size_t)p * D, norm64[p]);
                    mine = 1;
                }
            }
            if (!__syncthreads_or(mine)) continue;  // uniform: nothing of this chunk is admitted
            // candidates = this chunk's scores followed by the running list
            block_select<MIX_THREADS>(cn + k, k,
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
            part_s[((size_t)blockIdx.x * C + q) * k + tid] = run_s[tid];
            part_o[((size_t)blockIdx.x * C + q) * k + tid] = run_o[tid];
        }
    }
}

// ---- the winning term ----------------------------------------------------------------------------------------
// T of the rows a fold returned, after either path (finalize or redo merge wrote out_rows in this stream): one block per
// query, one (returned row, term) cosine per thread and step, then fold_terms per row.  A row id is mapped back through
// row_stride / row_offset; -1 stays -1, and an id that is no live row (none is written by this call) gives -1, never a
// read outside the store.  Dynamic LDS: the J terms.
template <int DT, int OP>
__global__ void __launch_bounds__(MIX_THREADS)
    fold_terms_kernel(const uint16_t *__restrict__ mem, const double *__restrict__ norm64,
                      const uint16_t *__restrict__ tiles, const double *__restrict__ weights,
                      const double *__restrict__ qn, const int64_t *__restrict__ d_total, int64_t cap, int ring, int D,
                      int J, int k, int64_t row_stride, int64_t row_offset, const int64_t *__restrict__ out_rows,
                      int *__restrict__ out_terms) {
    extern __shared__ __attribute__((aligned(16))) char ft_dyn[];
    uint16_t *tl = reinterpret_cast<uint16_t *>(ft_dyn);  // [J][D]
    __shared__ double ec[SKMAX * MIX_J];
    __shared__ int64_t ord[SKMAX];
    __shared__ double wl[MIX_J], ql[MIX_J];
    const int q = blockIdx.x, tid = threadIdx.x;
    const RingView rv = ring_view(*d_total, cap, ring);
    for (int i = tid; i < J * (D / 8); i += MIX_THREADS)
        reinterpret_cast<uint4 *>(tl)[i] = reinterpret_cast<const uint4 *>(tiles + (size_t)q * MIX_J * D)[i];
    if (tid < k) {
        const int64_t id = out_rows[(size_t)q * k + tid];
        const int64_t o = id < 0 ? -1 : (id - row_offset) / row_stride - rv.base;
        ord[tid] = (o >= 0 && o < rv.n) ? o : -1;
    }
    if (tid >= MIX_THREADS - MIX_J) {
        const int j = tid - (MIX_THREADS - MIX_J);
        wl[j] = j < J ? weights[(size_t)q * J + j] : 0.0;
        ql[j] = qn[q * MIX_J + j];
    }
    __syncthreads();
    for (int i = tid; i < k * J; i += MIX_THREADS) {  // (returned row, term) pairs
        const int cd = i / J, j = i - cd * J;
        if (ord[cd] < 0) continue;
        const int64_t p = slot_of(rv, ord[cd]);
        ec[cd * MIX_J + j] = ref_cosine(ref_dot<DT>(tl + (size_t)j * D, mem + (size_t)p * D, D), ql[j], norm64[p]);
    }
    __syncthreads();
    if (tid < k) {
        int arg = -1;
        if (ord[tid] >= 0) fold_terms<OP>(wl, [&](int j) { return ec[tid * MIX_J + j]; }, J, arg);
        out_terms[(size_t)q * k + tid] = arg;
    }
}

// ---- host --------------------------------------------------------------------------------------------------
// vm_key_image_plan for C key rows, then what the pack leaves: the packed tiles, the coefficients, the term norms, A and the
// domain flags
struct MPlan : SPlan {
    ScanGeom scan;  // the tile scan's grid: 16 C columns
    size_t off_tiles, off_coef, off_qn, off_A, off_dom, mix_total;
};

MPlan mix_plan(const vm_memory *m, int C, int k) {
    MPlan p;
    static_cast<SPlan &>(p) = vm_key_image_plan(m, C, k);
    p.scan = vm_scan_geom(m, C * MIX_J, (m->cap + 15) / 16, TS_THREADS);
    WsBump ws;
    ws.off = p.total;
    p.off_tiles = ws.take((size_t)C * MIX_J * m->D * 2);
    p.off_coef = ws.take((size_t)C * MIX_J * 4);
    p.off_qn = ws.take((size_t)C * MIX_J * 8);
    p.off_A = ws.take((size_t)C * 8);
    p.off_dom = ws.take((size_t)C * 4);
    p.mix_total = ws.off;
    return p;
}

// RowCall (queries = the terms [C][J][D], Q = C, score_mode raw) and what a mixed call adds to it
struct MixCall : RowCall {
    const double *weights;
    int J;
    const uint32_t *masks;  // null: every live row
    int n_masks;
    const int32_t *mask_index;
    size_t ws_bytes;
    bool fold;           // false: the mixed search (the sum), op is not read
    int op;              // a fold's vm_fold_op, as the caller gave it
    int32_t *out_terms;  // a fold's T [C][k], or null
};

constexpr int MIX_C_MAX = 1 << 20;  // 16 C columns and the workspace offsets stay far inside 32 bits of queries

int mix_check(vm_memory *m, const MixCall &c, const char *who) {
    vm_ctx *ctx = m->ctx;
    if (c.fold && c.op != VM_FOLD_MAX && c.op != VM_FOLD_MIN)
        return vm_fail(ctx, VM_ERR_INVALID, "%s: op=%d is no vm_fold_op", who, c.op);
    if (c.J < 1 || c.J > MIX_J) return vm_fail(ctx, VM_ERR_INVALID, "%s: J=%d outside [1, %d]", who, c.J, MIX_J);
    if (c.k < 1 || c.k > SKMAX) return vm_fail(ctx, VM_ERR_INVALID, "%s: k=%d outside [1, %d]", who, c.k, SKMAX);
    if (c.Q < 1 || c.Q > MIX_C_MAX) return vm_fail(ctx, VM_ERR_INVALID, "%s: C=%d outside [1, %d]", who, c.Q, MIX_C_MAX);
    if (!c.queries || !c.weights) return vm_fail(ctx, VM_ERR_INVALID, "%s: null terms or weights", who);
    if (!c.out_scores || !c.out_rows) return vm_fail(ctx, VM_ERR_INVALID, "%s: null outputs", who);
    if (c.row_stride < 1) return vm_fail(ctx, VM_ERR_INVALID, "%s: row_stride=%lld < 1", who, (long long)c.row_stride);
    if (c.masks)  // one mask per mixed query
        if (int rc = mask_operand_check(m, c.masks, c.n_masks, c.mask_index, c.Q, who)) return rc;
    const size_t need = mix_plan(m, c.Q, c.k).mix_total;
    if (!c.ws || c.ws_bytes < need) return vm_fail(ctx, VM_ERR_INVALID, "%s: workspace %zu < %zu", who, c.ws_bytes, need);
    if (((uintptr_t)c.ws & 255) || ((uintptr_t)c.queries & 15) || ((uintptr_t)c.weights & 7))
        return vm_fail(ctx, VM_ERR_INVALID, "%s: workspace must be 256-byte, terms 16-byte and weights 8-byte aligned",
                       who);
    return VM_OK;
}

// what both entries need of the workspace
struct MixBufs {
    uint16_t *tiles;
    float *coef;
    double *qn, *A;
    int *dom, *flags;
};
MixBufs mix_bufs(const MPlan &p, char *ws) {
    return {(uint16_t *)(ws + p.off_tiles), (float *)(ws + p.off_coef), (double *)(ws + p.off_qn),
            (double *)(ws + p.off_A),       (int *)(ws + p.off_dom),    (int *)(ws + p.off_flags)};
}

template <int DT, int OP>
int mix_pack(vm_memory *m, const MixCall &c, const MixBufs &b) {
    mix_pack_kernel<DT, OP><<<c.Q, MIX_THREADS, 0, c.stream>>>((const uint16_t *)c.queries, c.weights, c.J, m->D, b.tiles,
                                                         b.coef, b.qn, b.A, b.dom);
    VM_LAUNCH_CHECK(m->ctx);
    return VM_OK;
}

template <int DT, int OP, class P>
int mix_redo(vm_memory *m, const MPlan &p, const MixCall &c, const MixBufs &b, const P &pred) {
    vm_prof_scope prof(m->ctx, VM_PROF_TOPK_EXACT, c.stream);
    double *part_s = (double *)(c.ws + p.off_ps);
    int64_t *part_o = (int64_t *)(c.ws + p.off_po);
    const size_t lds = (size_t)c.J * m->D * 2;   // the J terms in dynamic LDS (the kernels' static arrays beside them)
    auto kern = mix_redo_scan_kernel<DT, OP, P>;
    if (int rc = vm_lds_opt_in(m->ctx, kern, lds, "vm_topk_cosine_mix")) return rc;
    kern<<<p.nblk, MIX_THREADS, lds, c.stream>>>(b.tiles, c.weights, b.qn, m->rows, m->norm64, m->d_total, m->cap,
                                                 m->ring, m->D, c.Q, c.J, c.k, b.flags, part_s, part_o, pred);
    VM_LAUNCH_CHECK(m->ctx);
    return vm_topk_redo_merge(m, part_s, part_o, p.nblk, c.Q, c.k, b.flags, c.use_min, c.min_score, VM_SCORE_RAW,
                              c.row_stride, c.row_offset, c.out_scores, c.out_rows, nullptr, nullptr, c.stream);
}

// a fold's T of the rows the call returned, when the caller wants it
template <int DT, int OP>
int fold_terms_out(vm_memory *m, const MixCall &c, const MixBufs &b) {
    if constexpr (OP != MIX_OP_SUM) {
        if (!c.out_terms) return VM_OK;
        const size_t lds = (size_t)c.J * m->D * 2;
        auto kern = fold_terms_kernel<DT, OP>;
        if (int rc = vm_lds_opt_in(m->ctx, kern, lds, "vm_topk_cosine_mix")) return rc;
        kern<<<c.Q, MIX_THREADS, lds, c.stream>>>(m->rows, m->norm64, b.tiles, c.weights, b.qn, m->d_total, m->cap,
                                                  m->ring, m->D, c.J, c.k, c.row_stride, c.row_offset, c.out_rows,
                                                  c.out_terms);
        VM_LAUNCH_CHECK(m->ctx);
    }
    return VM_OK;
}

// pack -> scan -> cut -> compact -> select -> finalize -> redo, or (exact) pack -> every query flagged -> redo; a fold
// then writes its T
template <int DT, int OP>
int mix_run(vm_memory *m, const MixCall &c, bool exact) {
    vm_ctx *ctx = m->ctx;
    hipStream_t st = c.stream;
    char *ws = c.ws;
    const int C = c.Q;
    const MPlan p = mix_plan(m, C, c.k);
    const MixBufs b = mix_bufs(p, ws);
    const MaskSel ms = {c.masks, c.mask_index, c.n_masks, mask_words(m)};
    if (!exact) {
        uint32_t *F = (uint32_t *)ws;
        {
            vm_prof_scope prof(ctx, VM_PROF_TOPK_SCAN, st);
            if (int rc = mix_pack<DT, OP>(m, c, b)) return rc;
            if constexpr (OP == MIX_OP_SUM) {
                const MixScan::Args a = {ms, b.coef, p.fstride, F};
                if (int rc = vm_tile_scan<DT, MixScan>(m, p.scan, b.tiles, C * MIX_J, a, st)) return rc;
            } else {
                const typename FoldScan<OP>::Args a = {{ms, b.coef, p.fstride, F}, c.J};
                if (int rc = vm_tile_scan<DT, FoldScan<OP>>(m, p.scan, b.tiles, C * MIX_J, a, st)) return rc;
            }
        }
        {
            vm_prof_scope prof(ctx, VM_PROF_TOPK_FINALIZE, st);
            if (int rc = vm_key_image_select(m, p, F, C, ws, st)) return rc;
            const size_t lds = (size_t)c.J * m->D * 2;
            auto kern = mix_finalize_kernel<DT, OP>;
            if (int rc = vm_lds_opt_in(m->ctx, kern, lds, "vm_topk_cosine_mix")) return rc;
            kern<<<C, MIX_THREADS, lds, st>>>(m->rows, m->norm64, b.tiles, c.weights, b.qn, b.A, b.dom, m->d_total,
                                              m->cap, m->ring, m->D, c.J, (const int *)(ws + p.off_co),
                                              (const uint32_t *)(ws + p.off_ck), (const int *)(ws + p.off_cn), p.M, c.k,
                                              c.use_min, c.min_score, c.row_stride, c.row_offset, c.out_scores, c.out_rows,
                                              c.out_uncertified, b.flags, c.out_query_flags);
            VM_LAUNCH_CHECK(ctx);
        }
    } else {
        if (int rc = mix_pack<DT, OP>(m, c, b)) return rc;
        if (int rc = vm_fill_flags(m, b.flags, C, st)) return rc;
    }
    if (int rc = c.masks ? mix_redo<DT, OP>(m, p, c, b, MaskScope{ms}) : mix_redo<DT, OP>(m, p, c, b, NoScope{})) return rc;
    return fold_terms_out<DT, OP>(m, c, b);
}

int mix_entry(vm_memory *m, const MixCall &c, bool exact, const char *who) {
    if (!m) return VM_ERR_INVALID;
    if (int rc = mix_check(m, c, who)) return rc;
    return vm_by_dtype(m, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (!c.fold) return mix_run<DT, MIX_OP_SUM>(m, c, exact);
        return c.op == VM_FOLD_MAX ? mix_run<DT, VM_FOLD_MAX>(m, c, exact) : mix_run<DT, VM_FOLD_MIN>(m, c, exact);
    });
}

}  // namespace

extern "C" size_t vm_topk_mix_workspace_bytes(const vm_memory *m, int C, int k) {
    if (!m || C < 1 || C > MIX_C_MAX || k < 1 || k > SKMAX) return 0;
    return mix_plan(m, C, k).mix_total;
}

extern "C" int vm_topk_cosine_mix(vm_memory *m, const void *terms, const double *weights, int C, int J, int k,
                                  const uint32_t *masks, int n_masks, const int32_t *mask_index, int use_min_score,
                                  double min_score, int64_t row_stride, int64_t row_offset, double *out_scores,
                                  int64_t *out_rows, int32_t *out_uncertified, int32_t *out_query_flags,
                                  void *workspace, size_t workspace_bytes, void *stream) {
    const MixCall c = {{terms, C, k, use_min_score, min_score, VM_SCORE_RAW, row_stride, row_offset, out_scores, out_rows,
                        out_uncertified, out_query_flags, (char *)workspace, (hipStream_t)stream},
                       weights, J, masks, n_masks, mask_index, workspace_bytes, false, 0, nullptr};
    return mix_entry(m, c, false, "vm_topk_cosine_mix");
}

extern "C" int vm_topk_cosine_mix_exact(vm_memory *m, const void *terms, const double *weights, int C, int J, int k,
                                        const uint32_t *masks, int n_masks, const int32_t *mask_index,
                                        int use_min_score, double min_score, int64_t row_stride, int64_t row_offset,
                                        double *out_scores, int64_t *out_rows, void *workspace, size_t workspace_bytes,
                                        void *stream) {
    const MixCall c = {{terms, C, k, use_min_score, min_score, VM_SCORE_RAW, row_stride, row_offset, out_scores, out_rows,
                        nullptr, nullptr, (char *)workspace, (hipStream_t)stream},
                       weights, J, masks, n_masks, mask_index, workspace_bytes, false, 0, nullptr};
    return mix_entry(m, c, true, "vm_topk_cosine_mix_exact");
}

extern "C" size_t vm_topk_fold_workspace_bytes(const vm_memory *m, int C, int k) {
    return vm_topk_mix_workspace_bytes(m, C, k);
}

extern "C" int vm_topk_cosine_fold(vm_memory *m, const void *terms, const double *weights, int C, int J, int k, int op,
                                   const uint32_t *masks, int n_masks, const int32_t *mask_index, int use_min_score,
                                   double min_score, int64_t row_stride, int64_t row_offset, double *out_scores,
                                   int64_t *out_rows, int32_t *out_terms, int32_t *out_uncertified,
                                   int32_t *out_query_flags, void *workspace, size_t workspace_bytes, void *stream) {
    const MixCall c = {{terms, C, k, use_min_score, min_score, VM_SCORE_RAW, row_stride, row_offset, out_scores, out_rows,
                        out_uncertified, out_query_flags, (char *)workspace, (hipStream_t)stream},
                       weights, J, masks, n_masks, mask_index, workspace_bytes, true, op, out_terms};
    return mix_entry(m, c, false, "vm_topk_cosine_fold");
}

extern "C" int vm_topk_cosine_fold_exact(vm_memory *m, const void *terms, const double *weights, int C, int J, int k,
                                         int op, const uint32_t *masks, int n_masks, const int32_t *mask_index,
                                         int use_min_score, double min_score, int64_t row_stride, int64_t row_offset,
                                         double *out_scores, int64_t *out_rows, int32_t *out_terms, void *workspace,
                                         size_t workspace_bytes, void *stream) {
    const MixCall c = {{terms, C, k, use_min_score, min_score, VM_SCORE_RAW, row_stride, row_offset, out_scores, out_rows,
                        nullptr, nullptr, (char *)workspace, (hipStream_t)stream},
                       weights, J, masks, n_masks, mask_index, workspace_bytes, true, op, out_terms};
    return mix_entry(m, c, true, "vm_topk_cosine_fold_exact");
}
