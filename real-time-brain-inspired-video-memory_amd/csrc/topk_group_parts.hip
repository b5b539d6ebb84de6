// The two kernels the grouped search (topk_group.hip) and the scoped grouped search (topk_group_scope.hip) launch
// unchanged, compiled once, and their launchers (topk_group_parts.h).  Everything else the two searches
// share is a template over the search's predicate or scan policy and stays in the header.
#include "topk_group_parts.h"

namespace {

// ---- table -------------------------------------------------------------------------------------------------
// first_o[g] = age order of the first live row of live group g (g = ordinal - ord0), first_o[ng] = n; F[0, Q*ng) = 0;
// fill_flags: flags[0, Q) = 1 (the exhaustive-only entry point).  Grid-stride, any grid.
__global__ void __launch_bounds__(256)
    group_table_kernel(const int64_t *__restrict__ d_total, int64_t cap, int ring, const int64_t *__restrict__ gord,
                       int Q, int *__restrict__ first_o, uint32_t *__restrict__ F, int32_t *__restrict__ flags,
                       int fill_flags) {
    const GroupView gv = group_view(d_total, cap, ring, gord);
    const int64_t n = gv.rv.n;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t o = t0; o <= n; o += stride) {
        if (o == n) {
            first_o[gv.ng] = (int)n;
        } else {
            const int64_t g = gord[slot_of(gv.rv, o)] - gv.ord0;
            if (o == 0 || gord[slot_of(gv.rv, o - 1)] - gv.ord0 != g) first_o[g] = (int)o;
        }
    }
    if (F)
        for (int64_t i = t0; i < (int64_t)Q * gv.ng; i += stride) F[i] = 0;
    if (fill_flags)
        for (int64_t i = t0; i < Q; i += stride) flags[i] = 1;
}

// ---- select: compaction ------------------------------------------------------------------------------------------
// grid (slices, Q): wave-aggregated appends of every composite >= cut[q] to the query's buffer
__global__ void __launch_bounds__(CMP_THREADS)
    group_compact_kernel(const int64_t *__restrict__ d_total, int64_t cap, int ring, const int64_t *__restrict__ gord,
                         const uint32_t *__restrict__ F, const unsigned long long *__restrict__ cut,
                         int *__restrict__ ccount, unsigned long long *__restrict__ cbuf) {
    // hits gather in LDS first: one global atomic per block (one per wave with hits on a single counter per query
    // serialised behind each other: 0.29 ms at Q = 16 over 200 k groups)
    __shared__ unsigned long long lbuf[CMP_LCAP];
    __shared__ int lcnt, gbase;
    const int q = blockIdx.y, lane = threadIdx.x & 63;
    const GroupView gv = group_view(d_total, cap, ring, gord);
    const int64_t ng = gv.ng;
    const uint32_t *Fq = F + (size_t)q * ng;
    const unsigned long long c0 = cut[q];
    const int64_t stride = (int64_t)gridDim.x * CMP_THREADS;
    if (threadIdx.x == 0) lcnt = 0;
    __syncthreads();
    for (int64_t base = (int64_t)blockIdx.x * CMP_THREADS; base < ng; base += stride) {  // uniform per wave
        const int64_t g = base + threadIdx.x;
        unsigned long long c = 0;
        if (g < ng) c = composite(Fq[g], (int)g);
        const bool hit = g < ng && c >= c0;
        const unsigned long long bal = __ballot(hit);
        if (bal) {
            int pos0 = 0;
            if (lane == 0) pos0 = atomicAdd(&lcnt, __popcll(bal));
            pos0 = __shfl(pos0, 0, 64);
            const int pos = pos0 + __popcll(bal & ((1ull << lane) - 1ull));
            if (hit && pos < CMP_LCAP) lbuf[pos] = c;
        }
    }
    __syncthreads();
    const int nb = lcnt;
    if (threadIdx.x == 0) gbase = nb ? atomicAdd(&ccount[q], nb > CMP_LCAP ? SEL_CAP + 1 : nb) : 0;  // >: radix path
    __syncthreads();
    if (nb > CMP_LCAP) return;
    for (int i = threadIdx.x; i < nb; i += CMP_THREADS) {
        const int pos = gbase + i;
        if (pos < SEL_CAP) cbuf[(size_t)q * SEL_CAP + pos] = lbuf[i];
    }
}

}  // namespace

// ---- host --------------------------------------------------------------------------------------------------
int vm_group_table(vm_memory *m, int blocks, int Q, int *first_o, uint32_t *F, int32_t *flags, int fill_flags,
                   hipStream_t st) {
    group_table_kernel<<<blocks, 256, 0, st>>>(m->d_total, m->cap, m->ring, m->gord, Q, first_o, F, flags, fill_flags);
    VM_LAUNCH_CHECK(m->ctx);
    return VM_OK;
}

int vm_group_compact(vm_memory *m, int slices, int Q, const uint32_t *F, const unsigned long long *cut, int *ccount,
                     unsigned long long *cbuf, hipStream_t st) {
    group_compact_kernel<<<dim3(slices, Q), CMP_THREADS, 0, st>>>(m->d_total, m->cap, m->ring, m->gord, F, cut, ccount,
                                                                  cbuf);
    VM_LAUNCH_CHECK(m->ctx);
    return VM_OK;
}
