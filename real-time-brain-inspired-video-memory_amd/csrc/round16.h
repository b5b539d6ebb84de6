// round16: ONE round-to-nearest-even from fp64 to the bits of a 16-bit float (fp16 or bf16), on the integer bits of the
// double.  Used by the group summaries (summary.hip: c_j = round16(S_j / N)).  A cast through fp32 would round twice:
// 1 + 2^-11 + 2^-40 is above the fp16 halfway point and rounds to 1 + 2^-10, but fp32 drops the 2^-40, leaves the exact
// tie 1 + 2^-11, and the second rounding goes to the even 1.0.  Subnormal results are kept (the shift grows below the
// smallest normal exponent), the sign of zero is kept, overflow gives infinity, NaN stays NaN.
// Free of HIP headers so that a host-only unit test can compile it (tests/test_summary_cpu.py).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VM_HD __host__ __device__
#else
#define VM_HD
#endif

// MBITS stored mantissa bits, EBITS exponent bits of the 16-bit format (1 + EBITS + MBITS = 16)
template <int MBITS, int EBITS>
VM_HD inline uint16_t vm_round16_bits(double x) {
    uint64_t u;
    __builtin_memcpy(&u, &x, 8);
    const uint16_t sign = (uint16_t)((u >> 48) & 0x8000u);
    const int ef = (int)((u >> 52) & 0x7ff);
    const uint64_t frac = u & (((uint64_t)1 << 52) - 1);
    const uint16_t inf = (uint16_t)(((1u << EBITS) - 1) << MBITS);
    if (ef == 0x7ff) return (uint16_t)(sign | inf | (frac ? (1u << (MBITS - 1)) : 0u));
    if (ef == 0) return sign;  // zero, or an fp64 subnormal: far below half the smallest 16-bit subnormal
    const int bias = (1 << (EBITS - 1)) - 1;
    const int e = ef - 1023;           // x = 1.frac x 2^e
    const int emin = 1 - bias;         // the smallest normal exponent
    const uint64_t sig = frac | ((uint64_t)1 << 52);
    int shift = 52 - MBITS;
    if (e < emin) shift += emin - e;   // subnormal result: units of 2^(emin - MBITS)
    if (shift > 54) return sign;       // below half the smallest subnormal
    uint64_t q = sig >> shift;
    const uint64_t rem = sig & (((uint64_t)1 << shift) - 1), half = (uint64_t)1 << (shift - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;
    // normal: q in [2^MBITS, 2^(MBITS+1)], a carry moves into the exponent field by itself; subnormal: q is the field
    const uint64_t mag = e >= emin ? ((uint64_t)(e + bias) << MBITS) + (q - ((uint64_t)1 << MBITS)) : q;
    return (uint16_t)(sign | (mag >= inf ? inf : (uint16_t)mag));
}

VM_HD inline uint16_t vm_round16_f16(double x) { return vm_round16_bits<10, 5>(x); }
VM_HD inline uint16_t vm_round16_bf16(double x) { return vm_round16_bits<7, 8>(x); }
