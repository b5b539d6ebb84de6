// Erase: forget rows of the embedding memory and compact it in place (include/vidmem.h vm_memory_erase_scoped /
// vm_memory_erase_rows).  The reference has no counterpart: its store is a database whose rows are
// deleted by Cypher (src/components/neo4j_handler.py:229-242 only ever MERGEs); the contract is the build's own: the
// memory afterwards is, bit for bit, a fresh memory that was appended the survivors.
//
// A stable compaction of [n, D] 16-bit rows and up to five side columns.  Nothing is read on the host and no block ever
// waits for another: ordering comes from the stream alone.
//   1 mark     keep flag of every live row (scoped: tag against the ranges, held in LDS; rows: ones, then a scatter of
//              zeros from the id list)
//   2 scan     per 256-row chunk: count -> one block scans the chunk counts -> new id of every row; writes the header
//              (old and new row count), out_new_row_of and out_erased
//   3 move     per segment of S rows, in stream order: GATHER the segment's survivors (all columns) into the scratch, then
//              SCATTER the scratch to slots [base, base + count).  base + count never exceeds the segment's end and the
//              earlier segments are finished, so a slot is overwritten only after its old content was read.  A segment
//              whose destination ends at or below its own start cannot overlap itself: its gather writes the destination
//              directly and its scatter returns at once (decided on the device).  A segment in front of the first erased
//              row returns from both launches at once.
//   4 regroup  grouped memories: ordinals from the compacted key column (the scan of 2 over "key differs from the
//              previous row's"), then the group state
//   5 tail     zero [n', n) in every column, write the row counter
#include "vm_internal.h"

namespace {

constexpr int ERASE_CHUNK = 256;              // rows per scan chunk; a segment is a whole number of chunks
constexpr int ERASE_DEFAULT_SEGMENT = 65536;  // rows per move segment when the caller names none
constexpr int ERASE_SCOPE_TILE = 512;         // tag ranges held in LDS at a time
constexpr size_t ERASE_HEADER_BYTES = 256;

struct EraseHeader {
    int64_t n_old;   // rows before the call (0 when the guard refused)
    int64_t n_new;   // rows after it
    int64_t bad;     // 1: the device row count exceeded the capacity (a wrapped ring) - nothing is touched
};

struct EraseWorkspace {
    EraseHeader *hdr;
    uint8_t *keep;     // [cap256]
    int32_t *newid;    // [cap256] rows kept before this one
    int32_t *ccount;   // [nchunk]
    int32_t *cbase;    // [nchunk + 1] exclusive scan of ccount
    uint16_t *s_rows;  // one segment of every column
    double *s_norm;
    int64_t *s_tag;
    int64_t *s_key;
    float *s_rnorm;
    int64_t seg;       // rows per segment
};

inline int64_t erase_cap256(const vm_memory *m) { return (m->cap + ERASE_CHUNK - 1) / ERASE_CHUNK * ERASE_CHUNK; }
inline size_t erase_fixed_bytes(const vm_memory *m) {
    const size_t c = (size_t)erase_cap256(m), nchunk = c / ERASE_CHUNK;
    return ERASE_HEADER_BYTES + vm_align_up(c, 256) + vm_align_up(c * 4, 256) + vm_align_up(nchunk * 4, 256) +
           vm_align_up((nchunk + 1) * 4, 256);
}
inline size_t erase_row_bytes(const vm_memory *m) {   // scratch per segment row: rows, norm64, tag, key, rnorm32
    return (size_t)m->D * 2 + 8 + 8 + 8 + 4;
}
inline int64_t erase_max_segment(const vm_memory *m) {
    const int64_t dflt = VM_DEV_ENV("ERASE_SEGMENT", ERASE_DEFAULT_SEGMENT) / ERASE_CHUNK * ERASE_CHUNK;
    const int64_t c = erase_cap256(m);
    return dflt < c ? (dflt < ERASE_CHUNK ? ERASE_CHUNK : dflt) : c;
}
inline EraseWorkspace erase_carve(const vm_memory *m, void *ws, int64_t seg) {
    const size_t c = (size_t)erase_cap256(m), nchunk = c / ERASE_CHUNK;
    char *p = (char *)ws;
    EraseWorkspace w;
    w.hdr = (EraseHeader *)p;
    p += ERASE_HEADER_BYTES;
    w.keep = (uint8_t *)p;
    p += vm_align_up(c, 256);
    w.newid = (int32_t *)p;
    p += vm_align_up(c * 4, 256);
    w.ccount = (int32_t *)p;
    p += vm_align_up(nchunk * 4, 256);
    w.cbase = (int32_t *)p;
    p += vm_align_up((nchunk + 1) * 4, 256);
    w.s_rows = (uint16_t *)p;   // seg is a multiple of 256 rows: every column below starts 256-byte aligned
    p += (size_t)seg * m->D * 2;
    w.s_norm = (double *)p;
    p += (size_t)seg * 8;
    w.s_tag = (int64_t *)p;
    p += (size_t)seg * 8;
    w.s_key = (int64_t *)p;
    p += (size_t)seg * 8;
    w.s_rnorm = (float *)p;
    w.seg = seg;
    return w;
}

// live rows by the device counter; -1 when it exceeds the capacity (the guard)
__device__ __forceinline__ int64_t live_rows(const int64_t *d_total, int64_t cap) {
    const int64_t t = *d_total;
    return t > cap ? -1 : t;
}

// ---- 1 mark ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) erase_mark_scoped_kernel(const int64_t *__restrict__ tag,
                                                                const int64_t *__restrict__ lo,
                                                                const int64_t *__restrict__ hi, int n_scopes,
                                                                const int64_t *__restrict__ d_total, int64_t cap,
                                                                uint8_t *__restrict__ keep) {
    __shared__ int64_t s_lo[ERASE_SCOPE_TILE], s_hi[ERASE_SCOPE_TILE];
    const int64_t n = live_rows(d_total, cap);
    const int64_t r0 = (int64_t)blockIdx.x * 256;
    if (r0 >= n) return;   // block-uniform
    const int64_t r = r0 + threadIdx.x;
    const int64_t t = r < n ? tag[r] : 0;
    bool hit = false;
    for (int s0 = 0; s0 < n_scopes; s0 += ERASE_SCOPE_TILE) {
        const int m = n_scopes - s0 < ERASE_SCOPE_TILE ? n_scopes - s0 : ERASE_SCOPE_TILE;
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += 256) {
            s_lo[i] = lo[s0 + i];
            s_hi[i] = hi[s0 + i];
        }
        __syncthreads();
        for (int i = 0; i < m; ++i) hit |= s_lo[i] <= t && t <= s_hi[i];
    }
    if (r < n) keep[r] = hit ? 0 : 1;
}

__global__ void __launch_bounds__(256) erase_mark_all_kernel(const int64_t *__restrict__ d_total, int64_t cap,
                                                             uint8_t *__restrict__ keep) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < live_rows(d_total, cap)) keep[r] = 1;
}

__global__ void __launch_bounds__(256) erase_mark_ids_kernel(const int64_t *__restrict__ ids, int64_t n_ids,
                                                             const int64_t *__restrict__ d_total, int64_t cap,
                                                             uint8_t *__restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_ids) return;
    const int64_t id = ids[i];
    if (id >= 0 && id < live_rows(d_total, cap)) keep[id] = 0;   // duplicates store the same byte
}

// ---- 2 scan (also 4 regroup) -------------------------------------------------------------------------------------
// FLAG_KEEP: flag of row r = keep[r], over the rows before the call.  FLAG_OPENS: flag = "row r opens a group" over the
// compacted key column, rows [0, n_new) of the header.
enum { FLAG_KEEP = 0, FLAG_OPENS = 1 };

template <int MODE>
__device__ __forceinline__ int64_t scan_rows(const EraseHeader *hdr, const int64_t *d_total, int64_t cap) {
    return MODE == FLAG_KEEP ? live_rows(d_total, cap) : (hdr->bad ? -1 : hdr->n_new);
}
template <int MODE>
__device__ __forceinline__ int row_flag(int64_t r, int64_t n, const uint8_t *keep, const int64_t *gkey) {
    if (r >= n) return 0;
    if (MODE == FLAG_KEEP) return keep[r];
    return r == 0 || gkey[r] != gkey[r - 1];
}

// inclusive scan of one int per thread over a 256-thread block; returns the thread's inclusive value, *total the sum
__device__ __forceinline__ int block_scan_256(int v, int *total) {
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    __syncthreads();   // wsum of an earlier call has been read
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    int before = 0, all = 0;
    for (int i = 0; i < 4; ++i) {
        if (i < w) before += wsum[i];
        all += wsum[i];
    }
    *total = all;
    return x + before;
}

template <int MODE>
__global__ void __launch_bounds__(256) erase_count_kernel(const EraseHeader *__restrict__ hdr,
                                                          const int64_t *__restrict__ d_total, int64_t cap,
                                                          const uint8_t *__restrict__ keep,
                                                          const int64_t *__restrict__ gkey,
                                                          int32_t *__restrict__ ccount) {
    const int64_t n = scan_rows<MODE>(hdr, d_total, cap);
    const int64_t r0 = (int64_t)blockIdx.x * ERASE_CHUNK;
    if (r0 >= n) return;
    int total;
    block_scan_256(row_flag<MODE>(r0 + threadIdx.x, n, keep, gkey), &total);
    if (threadIdx.x == 0) ccount[blockIdx.x] = total;
}

// One block: exclusive scan of the live chunks' counts into cbase[0 .. nchunks] (cbase[nchunks] = the sum).
// FLAG_KEEP: writes the header and *out_erased.  FLAG_OPENS: writes the group state of the compacted memory - that of a
// fresh memory after one grouped append of the survivors: groups opened, last key, open iff there is a row.
template <int MODE>
__global__ void __launch_bounds__(256) erase_chunk_scan_kernel(EraseHeader *__restrict__ hdr,
                                                               int64_t *__restrict__ d_total, int64_t cap,
                                                               const int32_t *__restrict__ ccount,
                                                               int32_t *__restrict__ cbase,
                                                               const int64_t *__restrict__ gkey,
                                                               int64_t *__restrict__ out_erased) {
    const int64_t n = scan_rows<MODE>(hdr, d_total, cap);
    if (n < 0) {
        if (MODE == FLAG_KEEP && threadIdx.x == 0) {
            hdr->n_old = 0;
            hdr->n_new = 0;
            hdr->bad = 1;
            if (out_erased) *out_erased = -1;
        }
        return;
    }
    const int64_t nchunks = (n + ERASE_CHUNK - 1) / ERASE_CHUNK;
    int64_t carry = 0;
    for (int64_t c0 = 0; c0 < nchunks; c0 += 256) {
        const int64_t c = c0 + threadIdx.x;
        const int v = c < nchunks ? ccount[c] : 0;
        int total;
        const int incl = block_scan_256(v, &total);
        if (c < nchunks) cbase[c] = (int32_t)(carry + incl - v);
        carry += total;
    }
    if (threadIdx.x == 0) {
        cbase[nchunks] = (int32_t)carry;
        if (MODE == FLAG_KEEP) {
            hdr->n_old = n;
            hdr->n_new = carry;
            hdr->bad = 0;
            if (out_erased) *out_erased = n - carry;
        } else {
            d_total[VM_GSTATE_GROUPS] = carry;
            d_total[VM_GSTATE_LAST_KEY] = n > 0 ? gkey[n - 1] : 0;
            d_total[VM_GSTATE_OPEN] = n > 0 ? 1 : 0;
        }
    }
}

// FLAG_KEEP: newid[r] = kept rows before r, out_new_row_of[r] = newid or -1.  FLAG_OPENS: gord[r] = groups opened up to
// and including r, minus one.
template <int MODE>
__global__ void __launch_bounds__(256) erase_apply_kernel(const EraseHeader *__restrict__ hdr,
                                                          const int64_t *__restrict__ d_total, int64_t cap,
                                                          const uint8_t *__restrict__ keep,
                                                          const int64_t *__restrict__ gkey,
                                                          const int32_t *__restrict__ cbase,
                                                          int32_t *__restrict__ newid,
                                                          int64_t *__restrict__ out_new_row_of,
                                                          int64_t *__restrict__ gord) {
    const int64_t n = scan_rows<MODE>(hdr, d_total, cap);
    const int64_t r0 = (int64_t)blockIdx.x * ERASE_CHUNK;
    if (r0 >= n) return;
    const int64_t r = r0 + threadIdx.x;
    const int flag = row_flag<MODE>(r, n, keep, gkey);
    int total;
    const int incl = block_scan_256(flag, &total);
    if (r >= n) return;
    const int64_t base = cbase[blockIdx.x];
    if (MODE == FLAG_KEEP) {
        const int64_t id = base + incl - flag;
        newid[r] = (int32_t)id;
        if (out_new_row_of) out_new_row_of[r] = flag ? id : -1;
    } else {
        gord[r] = base + incl - 1;
    }
}

// ---- 3 move ------------------------------------------------------------------------------------------------------
struct SegPlan {
    int64_t r0, r1;      // the segment's live rows [r0, r1)
    int64_t base, cnt;   // its survivors go to slots [base, base + cnt)
    bool idle, direct;   // idle: nothing to move
};
__device__ __forceinline__ SegPlan seg_plan(const EraseHeader *hdr, const int32_t *cbase, int64_t seg_index, int64_t seg,
                                            int allow_direct) {
    SegPlan p;
    const int64_t n = hdr->n_old;
    p.r0 = seg_index * seg;
    p.r1 = p.r0 + seg < n ? p.r0 + seg : n;
    p.idle = true;
    p.direct = false;
    p.base = p.cnt = 0;
    if (p.r0 >= n) return p;
    p.base = cbase[p.r0 / ERASE_CHUNK];
    p.cnt = cbase[(p.r1 + ERASE_CHUNK - 1) / ERASE_CHUNK] - p.base;
    p.idle = p.cnt == 0 || (p.base == p.r0 && p.cnt == p.r1 - p.r0);   // all erased, or nothing erased up to here
    p.direct = allow_direct && p.base + p.cnt <= p.r0;
    return p;
}

struct Columns {
    uint16_t *rows;
    double *norm;
    float *rnorm;
    int64_t *tag;   // null when the memory has none
    int64_t *key;
};

// One wave per row, four consecutive rows in flight per wave, 16-byte accesses; 256 threads = 16 rows per block.
// Survivor r goes to position newid[r] of the destination: the scratch (position - base), or the memory itself (direct).
__global__ void __launch_bounds__(256) erase_gather_kernel(const EraseHeader *__restrict__ hdr,
                                                           const int32_t *__restrict__ cbase, int64_t seg_index,
                                                           int64_t seg, int allow_direct,
                                                           const uint8_t *__restrict__ keep,
                                                           const int32_t *__restrict__ newid, Columns mem, Columns scr,
                                                           int D) {
    const SegPlan p = seg_plan(hdr, cbase, seg_index, seg, allow_direct);
    if (p.idle) return;
    const int lane = threadIdx.x & 63;
    const int64_t first = p.r0 + ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
    if (first >= p.r1) return;
    const Columns dst = p.direct ? mem : scr;
    const int64_t shift = p.direct ? 0 : p.base;
    const int V = D / 8;
    const uint4 *s[4];
    uint4 *d[4];
    bool k[4];
    for (int j = 0; j < 4; ++j) {
        const int64_t r = first + j;
        k[j] = r < p.r1 && keep[r];
        const int64_t to = k[j] ? (int64_t)newid[r] - shift : 0;
        s[j] = reinterpret_cast<const uint4 *>(mem.rows + (size_t)(k[j] ? r : 0) * D);
        d[j] = reinterpret_cast<uint4 *>(dst.rows + (size_t)to * D);
        if (k[j] && lane == j) {   // the side columns of row j: lane j
            dst.norm[to] = mem.norm[r];
            dst.rnorm[to] = mem.rnorm[r];
            if (mem.tag) dst.tag[to] = mem.tag[r];
            if (mem.key) dst.key[to] = mem.key[r];
        }
    }
    for (int i = lane; i < V; i += 64) {
        uint4 v[4];
        for (int j = 0; j < 4; ++j)
            if (k[j]) v[j] = s[j][i];
        for (int j = 0; j < 4; ++j)
            if (k[j]) d[j][i] = v[j];
    }
}

// flat 16-byte copy, four loads in flight per thread
__device__ __forceinline__ void copy_vec16(uint4 *__restrict__ dst, const uint4 *__restrict__ src, int64_t nvec,
                                           int64_t tid, int64_t stride) {
    for (int64_t i = tid; i < nvec; i += 4 * stride) {
        uint4 v[4];
        for (int j = 0; j < 4; ++j)
            if (i + j * stride < nvec) v[j] = src[i + j * stride];
        for (int j = 0; j < 4; ++j)
            if (i + j * stride < nvec) dst[i + j * stride] = v[j];
    }
}

__global__ void __launch_bounds__(256) erase_scatter_kernel(const EraseHeader *__restrict__ hdr,
                                                            const int32_t *__restrict__ cbase, int64_t seg_index,
                                                            int64_t seg, int allow_direct, Columns mem, Columns scr,
                                                            int D) {
    const SegPlan p = seg_plan(hdr, cbase, seg_index, seg, allow_direct);
    if (p.idle || p.direct) return;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    copy_vec16(reinterpret_cast<uint4 *>(mem.rows + (size_t)p.base * D), reinterpret_cast<const uint4 *>(scr.rows),
               p.cnt * (D / 8), tid, stride);
    for (int64_t i = tid; i < p.cnt; i += stride) {
        mem.norm[p.base + i] = scr.norm[i];
        mem.rnorm[p.base + i] = scr.rnorm[i];
        if (mem.tag) mem.tag[p.base + i] = scr.tag[i];
        if (mem.key) mem.key[p.base + i] = scr.key[i];
    }
}

// ---- 5 tail ------------------------------------------------------------------------------------------------------
// Zero the vacated slots [n_new, n_old) of every column, then publish the row count.  Nothing in this launch reads the
// counter: the header holds both counts.
__global__ void __launch_bounds__(256) erase_tail_kernel(const EraseHeader *__restrict__ hdr, Columns mem,
                                                         int64_t *__restrict__ gord, int D,
                                                         int64_t *__restrict__ d_total) {
    if (hdr->bad) return;
    const int64_t n0 = hdr->n_new, n1 = hdr->n_old;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    uint4 *rows = reinterpret_cast<uint4 *>(mem.rows + (size_t)n0 * D);
    const int64_t nvec = (n1 - n0) * (D / 8);
    const uint4 zero = make_uint4(0, 0, 0, 0);
    for (int64_t i = tid; i < nvec; i += stride) rows[i] = zero;
    for (int64_t i = n0 + tid; i < n1; i += stride) {
        mem.norm[i] = 0.0;
        mem.rnorm[i] = 0.0f;
        if (mem.tag) mem.tag[i] = 0;
        if (mem.key) mem.key[i] = 0;
        if (gord) gord[i] = 0;
    }
    if (tid == 0) d_total[0] = n0;
}

__global__ void erase_nothing_kernel(int64_t *out_erased) { *out_erased = 0; }

int erase_check(vm_memory *m, const char *what, void *workspace, size_t workspace_bytes, int64_t *seg_out) {
    vm_ctx *ctx = m->ctx;
    if (m->ring && m->h_total > m->cap)
        return vm_fail(ctx, VM_ERR_UNSUPPORTED, "%s: the ring has wrapped (%lld rows appended, capacity %lld)", what,
                       (long long)m->h_total, (long long)m->cap);
    if (!workspace) return vm_fail(ctx, VM_ERR_INVALID, "%s: workspace is null", what);
    const size_t fixed = erase_fixed_bytes(m);
    int64_t seg = workspace_bytes > fixed ? (int64_t)((workspace_bytes - fixed) / erase_row_bytes(m)) : 0;
    seg = seg / ERASE_CHUNK * ERASE_CHUNK;
    if (seg < ERASE_CHUNK)
        return vm_fail(ctx, VM_ERR_NOMEM, "%s: workspace of %zu bytes holds fewer than %d rows of scratch", what,
                       workspace_bytes, ERASE_CHUNK);
    const int64_t most = erase_max_segment(m);
    *seg_out = seg < most ? seg : most;
    return VM_OK;
}

// everything behind the marks: scan, move, regroup, tail
int erase_compact(vm_memory *m, const EraseWorkspace &w, int64_t *out_new_row_of, int64_t *out_erased, hipStream_t st) {
    vm_ctx *ctx = m->ctx;
    const int64_t cap256 = erase_cap256(m);
    const unsigned chunks = (unsigned)(cap256 / ERASE_CHUNK);
    erase_count_kernel<FLAG_KEEP><<<chunks, 256, 0, st>>>(w.hdr, m->d_total, m->cap, w.keep, nullptr, w.ccount);
    erase_chunk_scan_kernel<FLAG_KEEP><<<1, 256, 0, st>>>(w.hdr, m->d_total, m->cap, w.ccount, w.cbase, nullptr,
                                                          out_erased);
    erase_apply_kernel<FLAG_KEEP><<<chunks, 256, 0, st>>>(w.hdr, m->d_total, m->cap, w.keep, nullptr, w.cbase, w.newid,
                                                          out_new_row_of, nullptr);
    VM_LAUNCH_CHECK(ctx);
    const Columns mem = {m->rows, m->norm64, m->rnorm32, m->tag, m->gkey};
    const Columns scr = {w.s_rows, w.s_norm, w.s_rnorm, w.s_tag, w.s_key};
    const int allow_direct = VM_DEV_ENV("ERASE_DIRECT", 1) != 0;
    const int64_t nseg = (cap256 + w.seg - 1) / w.seg;
    const unsigned ggrid = (unsigned)(w.seg / 16);
    int64_t sblocks = w.seg * (m->D / 8) / (256 * 4);   // four 16-byte pieces per thread
    if (sblocks > 4096) sblocks = 4096;
    if (sblocks < 1) sblocks = 1;
    for (int64_t s = 0; s < nseg; ++s) {
        erase_gather_kernel<<<ggrid, 256, 0, st>>>(w.hdr, w.cbase, s, w.seg, allow_direct, w.keep, w.newid, mem, scr,
                                                   m->D);
        erase_scatter_kernel<<<(unsigned)sblocks, 256, 0, st>>>(w.hdr, w.cbase, s, w.seg, allow_direct, mem, scr, m->D);
    }
    VM_LAUNCH_CHECK(ctx);
    if (m->gkey) {
        erase_count_kernel<FLAG_OPENS><<<chunks, 256, 0, st>>>(w.hdr, m->d_total, m->cap, nullptr, m->gkey, w.ccount);
        erase_chunk_scan_kernel<FLAG_OPENS><<<1, 256, 0, st>>>(w.hdr, m->d_total, m->cap, w.ccount, w.cbase, m->gkey,
                                                               nullptr);
        erase_apply_kernel<FLAG_OPENS><<<chunks, 256, 0, st>>>(w.hdr, m->d_total, m->cap, nullptr, m->gkey, w.cbase,
                                                               nullptr, nullptr, m->gord);
        VM_LAUNCH_CHECK(ctx);
    }
    erase_tail_kernel<<<1024, 256, 0, st>>>(w.hdr, mem, m->gord, m->D, m->d_total);
    VM_LAUNCH_CHECK(ctx);
    return VM_OK;
}

}  // namespace

extern "C" size_t vm_memory_erase_workspace_bytes(const vm_memory *m, int64_t segment_rows) {
    if (!m || segment_rows < 0) return 0;
    const int64_t most = erase_max_segment(m);
    int64_t seg = segment_rows ? (segment_rows + ERASE_CHUNK - 1) / ERASE_CHUNK * ERASE_CHUNK : most;
    if (seg > most) seg = most;
    return erase_fixed_bytes(m) + (size_t)seg * erase_row_bytes(m);
}

extern "C" int vm_memory_erase_scoped(vm_memory *m, const int64_t *scope_lo, const int64_t *scope_hi, int n_scopes,
                                      int64_t *out_new_row_of, int64_t *out_erased, void *workspace,
                                      size_t workspace_bytes, void *stream) {
    if (!m) return VM_ERR_INVALID;
    vm_ctx *ctx = m->ctx;
    if (!m->tag) return vm_fail(ctx, VM_ERR_INVALID, "vm_memory_erase_scoped: the memory is not tagged");
    if (n_scopes < 1 || !scope_lo || !scope_hi)
        return vm_fail(ctx, VM_ERR_INVALID, "vm_memory_erase_scoped: needs at least one scope");
    int64_t seg = 0;
    const int rc = erase_check(m, "vm_memory_erase_scoped", workspace, workspace_bytes, &seg);
    if (rc != VM_OK) return rc;
    const EraseWorkspace w = erase_carve(m, workspace, seg);
    hipStream_t st = (hipStream_t)stream;
    erase_mark_scoped_kernel<<<(unsigned)(erase_cap256(m) / 256), 256, 0, st>>>(m->tag, scope_lo, scope_hi, n_scopes,
                                                                                m->d_total, m->cap, w.keep);
    VM_LAUNCH_CHECK(ctx);
    return erase_compact(m, w, out_new_row_of, out_erased, st);
}

extern "C" int vm_memory_erase_rows(vm_memory *m, const int64_t *row_ids, int64_t n, int64_t *out_new_row_of,
                                    int64_t *out_erased, void *workspace, size_t workspace_bytes, void *stream) {
    if (!m) return VM_ERR_INVALID;
    vm_ctx *ctx = m->ctx;
    if (n < 0 || (n > 0 && !row_ids)) return vm_fail(ctx, VM_ERR_INVALID, "vm_memory_erase_rows: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {   // a no-op: only the count is written
        if (out_erased) {
            erase_nothing_kernel<<<1, 1, 0, st>>>(out_erased);
            VM_LAUNCH_CHECK(ctx);
        }
        return VM_OK;
    }
    if ((n + 255) / 256 > 0x7fffffff) return vm_fail(ctx, VM_ERR_UNSUPPORTED, "vm_memory_erase_rows: too many ids");
    int64_t seg = 0;
    const int rc = erase_check(m, "vm_memory_erase_rows", workspace, workspace_bytes, &seg);
    if (rc != VM_OK) return rc;
    const EraseWorkspace w = erase_carve(m, workspace, seg);
    erase_mark_all_kernel<<<(unsigned)(erase_cap256(m) / 256), 256, 0, st>>>(m->d_total, m->cap, w.keep);
    erase_mark_ids_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(row_ids, n, m->d_total, m->cap, w.keep);
    VM_LAUNCH_CHECK(ctx);
    return erase_compact(m, w, out_new_row_of, out_erased, st);
}
