// Embedding memory: resident [capacity, D] 16-bit rows + exact fp64 norms + fp32 reciprocal norms.
// Replaces the Chunk.embedding property store of the reference
// (src/components/neo4j_handler.py:229-242 append, src/components/pre_llm_injector.py:390-412 read-back).
#include "topk_common.h"
#include "vm_internal.h"

#include <climits>

// One block per appended row: coalesced 16-B copy of the row into its slot, then lane 0 accumulates the
// reference's norm exactly: sqrt(sum(b*b)) with one rounding per product and per partial sum, left to right
// (src/components/pre_llm_injector.py:383).  The slot comes from the DEVICE-side counter so a captured graph
// replays correctly.  dom: the memory's domain word, &d_total[VM_GSTATE_OUTSIDE] (written, so not through d_total).
template <int DT>
__global__ void __launch_bounds__(128) memory_append_kernel(const uint16_t *__restrict__ src, int B, int D,
                                                            uint16_t *__restrict__ rows,
                                                            double *__restrict__ norm64,
                                                            float *__restrict__ rnorm32,
                                                            const int64_t *__restrict__ d_total, int64_t cap,
                                                            int ring, int64_t *dom) {
    const int b = blockIdx.x;
    const int64_t total = *d_total;
    int64_t id = total + b;
    int64_t slot = ring ? (id % cap) : id;
    if (slot >= cap) return;  // non-ring overflow is rejected on the host; never write out of bounds
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src + (size_t)b * D);
    uint4 *d4 = reinterpret_cast<uint4 *>(rows + (size_t)slot * D);
    for (int i = threadIdx.x; i < D / 8; i += blockDim.x) d4[i] = s4[i];
    if (threadIdx.x == 0) {
        const double nrm = __dsqrt_rn(ref_sumsq<DT>(src + (size_t)b * D, D));
        norm64[slot] = nrm;
        rnorm32[slot] = nrm > 0.0 ? (float)(1.0 / nrm) : 0.0f;
        // the certificate's sticky domain word (vm_internal.h VM_GSTATE_OUTSIDE; fp16 norms cannot leave the domain)
        if (DT == VM_BF16 && cert_norm_outside(nrm)) *dom = 1;
    }
}

__global__ void memory_bump_kernel(int64_t *d_total, int B) { *d_total += B; }

// Grouped memories: key and group ordinal of every appended row (one block, launched between the row copy and the bump
// so that it sees the same device row count).  A row opens a new group when its key differs from the previous row's -
// for the first row of the call: from the last key of the previous call, unless that call was a plain append or there
// was none (VM_GSTATE_OPEN == 0).  keys == null (plain append): every row is its own group, key = -1 - row id.
// Ordinal of a row = groups opened before it minus one, from an inclusive block scan of the "opens" flags.
__global__ void __launch_bounds__(256) memory_group_kernel(const int64_t *__restrict__ keys, int B, int64_t *__restrict__ gkey,
                                                           int64_t *__restrict__ gord, int64_t *__restrict__ state,
                                                           int64_t cap, int ring) {
    __shared__ int scan[256];
    const int tid = threadIdx.x;
    const int64_t total = state[0];
    int64_t groups = state[VM_GSTATE_GROUPS];
    const int64_t last_key = state[VM_GSTATE_LAST_KEY];
    const bool open = state[VM_GSTATE_OPEN] != 0;
    for (int c0 = 0; c0 < B; c0 += 256) {
        const int i = c0 + tid;
        int64_t kv = 0;
        int flag = 0;
        if (i < B) {
            kv = keys ? keys[i] : -1 - (total + i);
            if (!keys)
                flag = 1;
            else if (i == 0)
                flag = !(open && kv == last_key);
            else
                flag = keys[i - 1] != kv;
        }
        scan[tid] = flag;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int v = tid >= off ? scan[tid - off] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        if (i < B) {
            const int64_t id = total + i;
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
        state[VM_GSTATE_GROUPS] = groups;
        state[VM_GSTATE_LAST_KEY] = keys ? keys[B - 1] : 0;
        state[VM_GSTATE_OPEN] = keys ? 1 : 0;
    }
}

// Tagged memories: the tag of every appended row, into the slot the row copy used (launched before the bump, so it
// sees the same device row count).  tags == null (an append without tags): INT64_MIN.
__global__ void __launch_bounds__(256) memory_tag_kernel(const int64_t *__restrict__ tags, int B,
                                                         int64_t *__restrict__ tag, const int64_t *__restrict__ d_total,
                                                         int64_t cap, int ring) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const int64_t id = *d_total + i;
    const int64_t slot = ring ? id % cap : id;
    if (slot < cap) tag[slot] = tags ? tags[i] : LLONG_MIN;
}

extern "C" int vm_memory_create(vm_ctx *ctx, int64_t capacity_rows, int D, int dtype, int ring,
                                vm_memory **out) {
    if (!ctx || !out) return VM_ERR_INVALID;
    if (capacity_rows <= 0 || capacity_rows >= (int64_t)0x7fffff00)
        return vm_fail(ctx, VM_ERR_INVALID, "capacity_rows %lld out of range", (long long)capacity_rows);
    if (D <= 0 || D % 128 != 0)
        return vm_fail(ctx, VM_ERR_UNSUPPORTED, "D=%d: embedding dimension must be a multiple of 128", D);
    if (dtype != VM_F16 && dtype != VM_BF16) return vm_fail(ctx, VM_ERR_INVALID, "bad dtype %d", dtype);
    VM_HIP(ctx, hipSetDevice(ctx->device));
    vm_memory *m = new vm_memory();
    memset(m, 0, sizeof(*m));
    m->ctx = ctx;
    m->cap = capacity_rows;
    m->D = D;
    m->dtype = dtype;
    m->ring = ring ? 1 : 0;
    const int64_t cap_pad = (capacity_rows + 63) / 64 * 64;  // tail tiles may read (never use) past cap
    hipError_t e = hipMalloc((void **)&m->rows, (size_t)cap_pad * D * 2);
    if (e == hipSuccess) e = hipMalloc((void **)&m->norm64, (size_t)cap_pad * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&m->rnorm32, (size_t)cap_pad * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&m->d_total, 64);
    if (e != hipSuccess) {
        vm_memory_destroy(m);
        return vm_fail(ctx, VM_ERR_NOMEM, "hipMalloc for %lld x %d memory failed: %s", (long long)capacity_rows,
                       D, hipGetErrorString(e));
    }
    VM_HIP(ctx, hipMemset(m->rows, 0, (size_t)cap_pad * D * 2));
    VM_HIP(ctx, hipMemset(m->norm64, 0, (size_t)cap_pad * 8));
    VM_HIP(ctx, hipMemset(m->rnorm32, 0, (size_t)cap_pad * 4));
    VM_HIP(ctx, hipMemset(m->d_total, 0, 64));
    *out = m;
    return VM_OK;
}

extern "C" void vm_memory_destroy(vm_memory *m) {
    if (!m) return;
    if (m->rows) (void)hipFree(m->rows);
    if (m->norm64) (void)hipFree(m->norm64);
    if (m->rnorm32) (void)hipFree(m->rnorm32);
    if (m->d_total) (void)hipFree(m->d_total);
    if (m->gkey) (void)hipFree(m->gkey);
    if (m->gord) (void)hipFree(m->gord);
    if (m->tag) (void)hipFree(m->tag);
    delete m;
}

extern "C" int vm_memory_create_grouped(vm_ctx *ctx, int64_t capacity_rows, int D, int dtype, int ring,
                                        vm_memory **out) {
    vm_memory *m = nullptr;
    const int rc = vm_memory_create(ctx, capacity_rows, D, dtype, ring, &m);
    if (rc != VM_OK) return rc;
    const int64_t cap_pad = (capacity_rows + 63) / 64 * 64;
    hipError_t e = hipMalloc((void **)&m->gkey, (size_t)cap_pad * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&m->gord, (size_t)cap_pad * 8);
    if (e == hipSuccess) e = hipMemset(m->gkey, 0, (size_t)cap_pad * 8);
    if (e == hipSuccess) e = hipMemset(m->gord, 0, (size_t)cap_pad * 8);
    if (e != hipSuccess) {
        vm_memory_destroy(m);
        return vm_fail(ctx, VM_ERR_NOMEM, "group columns of a %lld-row memory: %s", (long long)capacity_rows,
                       hipGetErrorString(e));
    }
    *out = m;
    return VM_OK;
}

extern "C" int vm_memory_create_tagged(vm_ctx *ctx, int64_t capacity_rows, int D, int dtype, int ring, int grouped,
                                       vm_memory **out) {
    vm_memory *m = nullptr;
    const int rc = grouped ? vm_memory_create_grouped(ctx, capacity_rows, D, dtype, ring, &m)
                           : vm_memory_create(ctx, capacity_rows, D, dtype, ring, &m);
    if (rc != VM_OK) return rc;
    const int64_t cap_pad = (capacity_rows + 63) / 64 * 64;
    hipError_t e = hipMalloc((void **)&m->tag, (size_t)cap_pad * 8);
    if (e == hipSuccess) e = hipMemset(m->tag, 0, (size_t)cap_pad * 8);
    if (e != hipSuccess) {
        vm_memory_destroy(m);
        return vm_fail(ctx, VM_ERR_NOMEM, "tag column of a %lld-row memory: %s", (long long)capacity_rows,
                       hipGetErrorString(e));
    }
    *out = m;
    return VM_OK;
}

static int memory_append(vm_memory *m, const void *rows, int B, const int64_t *keys, const int64_t *tags,
                         int64_t *out_first_row_host, void *stream) {
    vm_ctx *ctx = m->ctx;
    if (B < 0 || (B > 0 && !rows)) return vm_fail(ctx, VM_ERR_INVALID, "vm_memory_append: bad arguments");
    if (out_first_row_host) *out_first_row_host = m->h_total;
    if (B == 0) return VM_OK;
    if (!m->ring && m->h_total + B > m->cap)
        return vm_fail(ctx, VM_ERR_NOMEM, "memory full: %lld + %d > capacity %lld", (long long)m->h_total, B,
                       (long long)m->cap);
    if (m->ring && B > m->cap) return vm_fail(ctx, VM_ERR_INVALID, "append of %d rows exceeds ring capacity", B);
    hipStream_t st = (hipStream_t)stream;
    vm_prof_scope prof(ctx, VM_PROF_APPEND, st);
    if (m->dtype == VM_F16)
        memory_append_kernel<VM_F16><<<B, 128, 0, st>>>((const uint16_t *)rows, B, m->D, m->rows, m->norm64,
                                                       m->rnorm32, m->d_total, m->cap, m->ring,
                                                        m->d_total + VM_GSTATE_OUTSIDE);
    else
        memory_append_kernel<VM_BF16><<<B, 128, 0, st>>>((const uint16_t *)rows, B, m->D, m->rows, m->norm64,
                                                        m->rnorm32, m->d_total, m->cap, m->ring,
                                                        m->d_total + VM_GSTATE_OUTSIDE);
    VM_LAUNCH_CHECK(ctx);
    if (m->gkey) {  // grouped memories only: a plain memory runs exactly the two launches above and below
        memory_group_kernel<<<1, 256, 0, st>>>(keys, B, m->gkey, m->gord, m->d_total, m->cap, m->ring);
        VM_LAUNCH_CHECK(ctx);
    }
    if (m->tag) {  // tagged memories only
        memory_tag_kernel<<<(B + 255) / 256, 256, 0, st>>>(tags, B, m->tag, m->d_total, m->cap, m->ring);
        VM_LAUNCH_CHECK(ctx);
    }
    memory_bump_kernel<<<1, 1, 0, st>>>(m->d_total, B);
    VM_LAUNCH_CHECK(ctx);
    m->h_total += B;
    return VM_OK;
}

extern "C" int vm_memory_append(vm_memory *m, const void *rows, int B, int64_t *out_first_row_host, void *stream) {
    if (!m) return VM_ERR_INVALID;
    return memory_append(m, rows, B, nullptr, nullptr, out_first_row_host, stream);
}

extern "C" int vm_memory_append_grouped(vm_memory *m, const void *rows, int B, const int64_t *keys,
                                        int64_t *out_first_row_host, void *stream) {
    if (!m) return VM_ERR_INVALID;
    if (!m->gkey) return vm_fail(m->ctx, VM_ERR_INVALID, "vm_memory_append_grouped: the memory is not grouped");
    if (B > 0 && !keys) return vm_fail(m->ctx, VM_ERR_INVALID, "vm_memory_append_grouped: keys is null");
    return memory_append(m, rows, B, keys, nullptr, out_first_row_host, stream);
}

extern "C" int vm_memory_append_tagged(vm_memory *m, const void *rows, int B, const int64_t *tags, const int64_t *keys,
                                       int64_t *out_first_row_host, void *stream) {
    if (!m) return VM_ERR_INVALID;
    if (!m->tag) return vm_fail(m->ctx, VM_ERR_INVALID, "vm_memory_append_tagged: the memory is not tagged");
    if (B > 0 && !tags) return vm_fail(m->ctx, VM_ERR_INVALID, "vm_memory_append_tagged: tags is null");
    if (keys && !m->gkey) return vm_fail(m->ctx, VM_ERR_INVALID, "vm_memory_append_tagged: keys on a memory that is not grouped");
    return memory_append(m, rows, B, keys, tags, out_first_row_host, stream);
}

extern "C" const int64_t *vm_memory_tags(const vm_memory *m) { return m ? m->tag : nullptr; }

extern "C" const int64_t *vm_memory_group_keys(const vm_memory *m) { return m ? m->gkey : nullptr; }

extern "C" int64_t vm_memory_size(const vm_memory *m) { return m ? m->h_total : 0; }
extern "C" int64_t vm_memory_capacity(const vm_memory *m) { return m ? m->cap : 0; }
extern "C" int vm_memory_dim(const vm_memory *m) { return m ? m->D : 0; }
extern "C" const void *vm_memory_rows(const vm_memory *m) { return m ? m->rows : nullptr; }

extern "C" int64_t vm_memory_sync(vm_memory *m, void *stream) {
    if (!m) return VM_ERR_INVALID;
    int64_t total = 0;
    VM_HIP(m->ctx, hipMemcpyAsync(&total, m->d_total, sizeof(total), hipMemcpyDeviceToHost, (hipStream_t)stream));
    VM_HIP(m->ctx, hipStreamSynchronize((hipStream_t)stream));
    m->h_total = total;
    return total;
}

extern "C" int vm_memory_reset(vm_memory *m, void *stream) {
    if (!m) return VM_ERR_INVALID;
    VM_HIP(m->ctx, hipMemsetAsync(m->d_total, 0, 64, (hipStream_t)stream));
    m->h_total = 0;
    return VM_OK;
}
