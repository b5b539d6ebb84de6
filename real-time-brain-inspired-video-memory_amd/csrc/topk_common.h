// The reference arithmetic, tie rule and certification bound of every top-k path ("Exactness").
//
// A top-k answer is the reference's bit for bit (src/components/pre_llm_injector.py:374-388): the fp64 cosine with one
// rounding per product and per partial sum, summed strictly left to right, the zero-norm guard and one division;
// results ordered by (score desc, row asc).  Each rule is defined here once; the row search (topk.hip), the exhaustive
// kernels (topk_exact.hip), the grouped and scoped searches (topk_group.hip, topk_scope.hip; their shared selection stage
// is topk_select.h) and the append's row norms (memory.hip) use it.
#pragma once
#include "vm_common.h"

// sum of v[i]^2 over [0, D), one rounding per product and per partial sum, strictly left to right; 16-byte reads.
// D is a multiple of 8.  The norm is __dsqrt_rn of it (src/components/pre_llm_injector.py:382-383).
template <int DT>
__device__ __forceinline__ double ref_sumsq(const uint16_t *v, int D) {
    using E = vm_elem<DT>;
    double s = 0.0;
    for (int i = 0; i < D; i += 8) {
        const uint4 a = *reinterpret_cast<const uint4 *>(v + i);
        const uint16_t *ae = reinterpret_cast<const uint16_t *>(&a);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double x = E::to_double(ae[j]);
            s = __dadd_rn(s, __dmul_rn(x, x));
        }
    }
    return s;
}

// sum of a[i] * b[i] over [0, D), rounded and ordered as ref_sumsq.  a: the query (usually in LDS), b: a stored row,
// read 4 chunks of 16 bytes ahead per step.  D is a multiple of 32 (memories keep D a multiple of 128).
template <int DT>
__device__ __forceinline__ double ref_dot(const uint16_t *a, const uint16_t *b, int D) {
    using E = vm_elem<DT>;
    double dot = 0.0;
    for (int i = 0; i < D; i += 32) {
        uint4 b4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) b4[u] = *reinterpret_cast<const uint4 *>(b + i + 8 * u);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint4 a4 = *reinterpret_cast<const uint4 *>(a + i + 8 * u);
            const uint16_t *ae = reinterpret_cast<const uint16_t *>(&a4);
            const uint16_t *be = reinterpret_cast<const uint16_t *>(&b4[u]);
#pragma unroll
            for (int j = 0; j < 8; ++j) dot = __dadd_rn(dot, __dmul_rn(E::to_double(ae[j]), E::to_double(be[j])));
        }
    }
    return dot;
}

// the cosine from the dot and the two norms: 0 when either vector is zero, else one division
// (src/components/pre_llm_injector.py:385-388)
__device__ __forceinline__ double ref_cosine(double dot, double qn, double mn) {
    return (qn == 0.0 || mn == 0.0) ? 0.0 : __ddiv_rn(dot, __dmul_rn(qn, mn));
}

// the score a caller sees for cosine e (include/vidmem.h vm_score_mode)
__device__ __forceinline__ double shown_score(double e, int score_mode) {
    return score_mode == VM_SCORE_UNIT_INTERVAL ? __ddiv_rn(__dadd_rn(1.0, e), 2.0) : e;
}

// the min_score filter: a hit is kept when its shown score is strictly above the threshold
__device__ __forceinline__ bool passes_min(int use_min, double shown, double min_score) {
    return !use_min || shown > min_score;
}

// Certification bound, DESIGN.md 4.1: an fp32-scanned score x 1/||q|| lies within 2 (D + 8) 2^-24 of the exact cosine,
// so an exact k-th score above (best rejected fp32 score / ||q||) + cert_eps(D) is provably the k-th.
// PRECONDITION ("Domain of the certificate"): the bound is a statement about fp32 arithmetic that neither
// overflows nor underflows.  It holds when the query's norm and the norm of EVERY stored row are 0 or lie in
// [2^-40, 2^40] (cert_norm_outside below) and D <= 2,048; a kernel that uses cert_eps must check that first and, outside,
// treat the query as uncertified (the row, grouped and scoped searches: VM_FLAG_GAP -> the exhaustive redo; the range
// search: every pair is a candidate).  Stored NaN / inf values are undefined, as in the reference.
__device__ __forceinline__ double cert_eps(int D) { return 2.0 * (double)(D + 8) * 5.9604644775390625e-08; }

// The norm interval of the certificate's domain.  fp16 norms cannot leave it (they lie in [2^-24, 2^22]); a bf16 norm
// can.  A zero vector is inside: its fp32 score is an exact 0.  A NaN norm is outside.
constexpr double VM_CERT_NORM_MIN = 9.094947017729282379150390625e-13;  // 2^-40
constexpr double VM_CERT_NORM_MAX = 1099511627776.0;                    // 2^40
__device__ __forceinline__ bool cert_norm_outside(double nrm) {
    return nrm != 0.0 && !(nrm >= VM_CERT_NORM_MIN && nrm <= VM_CERT_NORM_MAX);
}

// the tie rule of the fp32 candidate lists: (score desc, age order asc)
__device__ __forceinline__ bool better(float s1, int o1, float s2, int o2) {
    return s1 > s2 || (s1 == s2 && o1 < o2);
}

// k rounds of block-wide arg-best over n (score, order) candidates read through `get`, strictly after the previous
// winner in (score desc, order asc): a stable top-k without sorting.  Winners go to out_s / out_o (LDS), -inf / -1
// padded; a candidate with order < 0 is absent.  red_s / red_o: NT / 64 entries of LDS.  All NT threads of the block
// must call it.
template <int NT, typename Get>
__device__ __forceinline__ void block_select(int n, int k, Get get, double *out_s, int64_t *out_o, double *red_s,
                                             int64_t *red_o) {
    const int tid = threadIdx.x;
    double prev_s = INFINITY;
    int64_t prev_o = -1;
    for (int r = 0; r < k; ++r) {
        double bs = -INFINITY;
        int64_t bo = -1;
        for (int i = tid; i < n; i += NT) {
            double v;
            int64_t o;
            get(i, v, o);
            if (o < 0) continue;
            const bool after_prev = v < prev_s || (v == prev_s && o > prev_o);
            const bool beats = bo < 0 || v > bs || (v == bs && o < bo);
            if (after_prev && beats) {
                bs = v;
                bo = o;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double s2 = __shfl_xor(bs, off, 64);
            const int64_t o2 = __shfl_xor(bo, off, 64);
            if (o2 >= 0 && (bo < 0 || s2 > bs || (s2 == bs && o2 < bo))) {
                bs = s2;
                bo = o2;
            }
        }
        __syncthreads();  // previous round's readers of red_* are done
        if ((tid & 63) == 0) {
            red_s[tid >> 6] = bs;
            red_o[tid >> 6] = bo;
        }
        __syncthreads();
        bs = red_s[0];
        bo = red_o[0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) {
            const double s2 = red_s[w];
            const int64_t o2 = red_o[w];
            if (o2 >= 0 && (bo < 0 || s2 > bs || (s2 == bs && o2 < bo))) {
                bs = s2;
                bo = o2;
            }
        }
        if (tid == 0) {
            out_s[r] = bo >= 0 ? bs : -INFINITY;
            out_o[r] = bo;
        }
        prev_s = bs;
        prev_o = bo;
        if (bo < 0) {  // exhausted (uniform): pad the rest
            for (int r2 = r + 1 + tid; r2 < k; r2 += NT) {
                out_s[r2] = -INFINITY;
                out_o[r2] = -1;
            }
            break;
        }
    }
    __syncthreads();
}
