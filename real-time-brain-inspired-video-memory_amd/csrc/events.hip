// Event segmentation: cut the stored rows into EVENTS, maximal runs of consecutive row ids in which every frame
// resembles the one before it (include/vidmem.h vm_memory_events / vm_memory_regroup_events).  The
// reference has no counterpart: it stores one text embedding per fixed chunk (src/components/neo4j_handler.py:229-242)
// and cuts a video every chunk_size_seconds (src/pipeline/vlm_extractor.py:38-46), whatever it shows.
//
// link(r) = the reference cosine of rows r - 1 and r (topk_common.h: fp64 on the stored 16-bit values, one rounding per
// product and per partial sum, left to right, the stored norms, the zero-norm guard); row r opens an event when it is
// the oldest live row, when !(link(r) > threshold), or when the tags of the two rows say so (ev_opens).  There is no
// matrix structure - one exact pair per row - so there is no fp32 stage, nothing to certify and nothing to redo.
//   link    : one lane per pair - the exact dot is strictly sequential - and 256 consecutive age orders per block: the
//             link, the "opens" flag, and the block's flag count and last flagged row.  The bytes reach the lane
//             through LDS: the block's 256 rows plus the row before them (the halo) are loaded slice by slice of 64
//             elements with coalesced 16-byte loads (8 lanes = one 128-byte line of a row) into two buffers, the next
//             slice's loads in flight while this one is summed; every lane carries its fp64 sum across the slices.
//             Every row is read once, plus 1/256 for the halo.
//   scan    : one block: exclusive prefix of the chunk counts, running "last flagged row before this chunk"; the event
//             count; for a regroup the group state
//   apply   : per chunk the inclusive scans of the flags (sum: event index, max: the event's first row), then either
//             the outputs of vm_memory_events or the key and ordinal columns
// Order comes from prefix sums over separate launches: no atomics, no workgroup waits for another.  Every launch reads
// the row count from the device and is sized from the capacity.
#include "topk_common.h"
#include "vm_internal.h"

#include <climits>
#include <cmath>

namespace {

constexpr int EV_CHUNK = 256;  // age orders per block of every launch
constexpr size_t EV_HEADER_BYTES = 256;
constexpr int64_t EV_MS_MASK = ((int64_t)1 << 40) - 1;

struct EvHeader {
    int64_t n_events;  // flags among the covered rows
};

// The rows a call covers, as age orders [o0, rv.n): everything (whole mode) or the rows from *from_row on (tail mode).
// o0 == rv.n: nothing to do (an empty memory, or *from_row at or beyond the row count).
struct EvSpan {
    RingView rv;
    int64_t o0;
    bool tail;  // o0 > 0: row o0 is judged against its predecessor and inherits from it
};
__device__ __forceinline__ EvSpan ev_span(const int64_t *d_total, int64_t cap, int ring, const int64_t *from_row) {
    EvSpan s;
    s.rv = ring_view(*d_total, cap, ring);
    s.o0 = 0;
    if (from_row) {
        const int64_t from = *from_row;
        if (from > s.rv.base) s.o0 = from - s.rv.base < s.rv.n ? from - s.rv.base : s.rv.n;
    }
    s.tail = s.o0 > 0;
    return s;
}

// Does the row in slot sc open an event after the row in slot sp?  The score rule, then on a tagged memory the tag
// rules: exactly one untimed row (INT64_MIN), another source, or - max_gap_ms >= 0 - time running backwards or jumping.
__device__ __forceinline__ bool ev_opens(double link, double threshold, const int64_t *__restrict__ tag, int64_t sp,
                                         int64_t sc, int64_t max_gap_ms) {
    bool opens = !(link > threshold);
    if (tag) {
        const int64_t tp = tag[sp], tc = tag[sc];
        const bool up = tp == LLONG_MIN, uc = tc == LLONG_MIN;
        if (up != uc) {
            opens = true;
        } else if (!up) {
            const int64_t step = (tc & EV_MS_MASK) - (tp & EV_MS_MASK);
            if ((tp >> 40) != (tc >> 40) || (max_gap_ms >= 0 && (step < 0 || step > max_gap_ms))) opens = true;
        }
    }
    return opens;
}

// inclusive scans of one (count, last position) pair per thread over a 256-thread block: sum and max
struct EvScan {
    int sum, last;
};
__device__ __forceinline__ EvScan ev_block_scan(int v, int last, int *s_sum, int *s_last) {
    const int tid = threadIdx.x;
    __syncthreads();  // readers of an earlier call are done
    s_sum[tid] = v;
    s_last[tid] = last;
    __syncthreads();
    for (int off = 1; off < EV_CHUNK; off <<= 1) {
        const int a = tid >= off ? s_sum[tid - off] : 0;
        const int b = tid >= off ? s_last[tid - off] : -1;
        __syncthreads();
        s_sum[tid] += a;
        if (b > s_last[tid]) s_last[tid] = b;
        __syncthreads();
    }
    EvScan r;
    r.sum = s_sum[tid];
    r.last = s_last[tid];
    return r;
}

// ---- link, the simple form -----------------------------------------------------------------------------------------
// Every lane runs ref_dot on global memory, as range.hip's rescore does.  Kept as the yardstick of the streamed form and
// compiled into the developer library only (vm_common.h, VM_DEV_ENV): VIDMEM_EVENTS_SIMPLE=1 in libvidmem_dev.so,
// tools/event_probe.py.
// Block c owns the age orders [256 c, 256 c + 256).  flags[o] = row o opens an event; ccount[c] / clast[c] = the
// chunk's flags and its last flagged age order (-1: none), over the covered rows only.
#ifdef VM_DEV_SWITCHES
template <int DT>
__global__ void __launch_bounds__(EV_CHUNK)
    events_link_kernel(const uint16_t *__restrict__ rows, const double *__restrict__ norm64,
                       const int64_t *__restrict__ tag, const int64_t *__restrict__ d_total, int64_t cap, int ring,
                       int D, const int64_t *__restrict__ from_row, double threshold, int64_t max_gap_ms,
                       double *__restrict__ out_links, uint8_t *__restrict__ flags, int32_t *__restrict__ ccount,
                       int32_t *__restrict__ clast) {
    __shared__ int s_sum[EV_CHUNK], s_last[EV_CHUNK];
    const EvSpan sp = ev_span(d_total, cap, ring, from_row);
    const int64_t n = sp.rv.n;
    const int64_t c0 = (int64_t)blockIdx.x * EV_CHUNK;
    if (c0 >= n || c0 + EV_CHUNK <= sp.o0) return;  // block-uniform: no covered row here
    const int64_t o = c0 + threadIdx.x;
    int flag = 0;
    if (o < n && o >= sp.o0) {
        double link = 0.0;
        bool opens = true;
        if (o > 0) {
            const int64_t a = slot_of(sp.rv, o - 1), b = slot_of(sp.rv, o);
            link = ref_cosine(ref_dot<DT>(rows + (size_t)a * D, rows + (size_t)b * D, D), norm64[a], norm64[b]);
            opens = ev_opens(link, threshold, tag, a, b, max_gap_ms);
        }
        if (out_links) out_links[o] = link;
        flag = opens ? 1 : 0;
        flags[o] = (uint8_t)flag;
    }
    const EvScan r = ev_block_scan(flag, flag ? (int)o : -1, s_sum, s_last);
    if (threadIdx.x == EV_CHUNK - 1) {
        ccount[blockIdx.x] = r.sum;
        clast[blockIdx.x] = r.last;
    }
}
#endif  // VM_DEV_SWITCHES

// ---- link, streamed through LDS ------------------------------------------------------------------------------------
// LDS row j of a buffer holds the slice of age order 256 c - 1 + j (row 0: the halo); lane t sums rows t and t + 1.
// Row pitch 144 bytes = 9 slots of 16 bytes, an odd number: the 16 lanes of a ds_read_b128 group read 16 consecutive
// rows modulo 16 (its lane sets are 0-3, 12-15, 20-27 and the like), so their slots 9 t mod 16 are all different - no
// bank conflict; with the pitch of the data alone (128 bytes) every second row would start on the same bank.
constexpr int EV_SLICE = 64;                      // elements per stage
constexpr int EV_PIECES = EV_SLICE / 8;           // 16-byte pieces per row and stage
constexpr int EV_PITCH = EV_SLICE * 2 + 16;       // bytes
constexpr int EV_BUF = (EV_CHUNK + 1) * EV_PITCH; // one buffer
constexpr int EV_PER = EV_CHUNK * EV_PIECES / EV_CHUNK;  // pieces per thread and stage (the halo apart): 8
static_assert((EV_PITCH / 16) % 2 == 1, "an odd number of 16-byte slots per LDS row");

template <int DT>
__global__ void __launch_bounds__(EV_CHUNK)
    events_link_stream_kernel(const uint16_t *__restrict__ rows, const double *__restrict__ norm64,
                              const int64_t *__restrict__ tag, const int64_t *__restrict__ d_total, int64_t cap,
                              int ring, int D, const int64_t *__restrict__ from_row, double threshold,
                              int64_t max_gap_ms, double *__restrict__ out_links, uint8_t *__restrict__ flags,
                              int32_t *__restrict__ ccount, int32_t *__restrict__ clast) {
    using E = vm_elem<DT>;
    extern __shared__ __attribute__((aligned(16))) char ev_lds[];  // 2 x EV_BUF
    __shared__ int s_sum[EV_CHUNK], s_last[EV_CHUNK];
    const EvSpan sp = ev_span(d_total, cap, ring, from_row);
    const int64_t n = sp.rv.n;
    const int64_t c0 = (int64_t)blockIdx.x * EV_CHUNK;
    if (c0 >= n || c0 + EV_CHUNK <= sp.o0) return;  // block-uniform: no covered row here
    const int tid = threadIdx.x;
    // this thread's share of a stage: piece tid % 8 of the rows tid / 8 + 32 u; threads 0 - 7 also load the halo
    const int piece = tid % EV_PIECES, r0 = tid / EV_PIECES;
    const uint4 *src[EV_PER];
#pragma unroll
    for (int u = 0; u < EV_PER; ++u) {
        const int64_t o = c0 + r0 + (EV_CHUNK / EV_PER) * u;
        src[u] = o < n ? reinterpret_cast<const uint4 *>(rows + (size_t)slot_of(sp.rv, o) * D) + piece : nullptr;
    }
    const uint4 *src_halo = (tid < EV_PIECES && c0 > 0)
                                ? reinterpret_cast<const uint4 *>(rows + (size_t)slot_of(sp.rv, c0 - 1) * D) + tid
                                : nullptr;
    uint4 st[EV_PER], st_halo;
    auto load = [&](int s) {
#pragma unroll
        for (int u = 0; u < EV_PER; ++u) st[u] = src[u] ? src[u][s * EV_PIECES] : make_uint4(0, 0, 0, 0);
        st_halo = src_halo ? src_halo[s * EV_PIECES] : make_uint4(0, 0, 0, 0);
    };
    auto store = [&](int buf) {
        char *base = ev_lds + buf * EV_BUF;
#pragma unroll
        for (int u = 0; u < EV_PER; ++u)
            *reinterpret_cast<uint4 *>(base + (r0 + (EV_CHUNK / EV_PER) * u + 1) * EV_PITCH + piece * 16) = st[u];
        if (tid < EV_PIECES) *reinterpret_cast<uint4 *>(base + tid * 16) = st_halo;
    };
    const int nsl = D / EV_SLICE;
    load(0);
    store(0);
    __syncthreads();
    double dot = 0.0;
    for (int s = 0; s < nsl; ++s) {
        if (s + 1 < nsl) load(s + 1);  // in flight while this slice is summed
        const char *pa = ev_lds + (s & 1) * EV_BUF + tid * EV_PITCH, *pb = pa + EV_PITCH;
#pragma unroll
        for (int k = 0; k < EV_PIECES; ++k) {
            const uint4 a4 = *reinterpret_cast<const uint4 *>(pa + 16 * k);
            const uint4 b4 = *reinterpret_cast<const uint4 *>(pb + 16 * k);
            const uint16_t *ae = reinterpret_cast<const uint16_t *>(&a4);
            const uint16_t *be = reinterpret_cast<const uint16_t *>(&b4);
#pragma unroll
            for (int j = 0; j < 8; ++j) dot = __dadd_rn(dot, __dmul_rn(E::to_double(ae[j]), E::to_double(be[j])));
        }
        if (s + 1 < nsl) store((s + 1) & 1);  // last read two iterations ago, before the previous barrier
        __syncthreads();
    }
    const int64_t o = c0 + tid;
    int flag = 0;
    if (o < n && o >= sp.o0) {
        double link = 0.0;
        bool opens = true;
        if (o > 0) {
            const int64_t a = slot_of(sp.rv, o - 1), b = slot_of(sp.rv, o);
            link = ref_cosine(dot, norm64[a], norm64[b]);
            opens = ev_opens(link, threshold, tag, a, b, max_gap_ms);
        }
        if (out_links) out_links[o] = link;
        flag = opens ? 1 : 0;
        flags[o] = (uint8_t)flag;
    }
    const EvScan r = ev_block_scan(flag, flag ? (int)o : -1, s_sum, s_last);
    if (tid == EV_CHUNK - 1) {
        ccount[blockIdx.x] = r.sum;
        clast[blockIdx.x] = r.last;
    }
}

// ---- scan ------------------------------------------------------------------------------------------------------
// One block.  cbase[c] = flags in the covered chunks before c, cprev[c] = the last flagged age order before chunk c
// (-1: none).  Writes the event count; REGROUP: the group state - groups opened, the last row's key, closed.
__global__ void __launch_bounds__(EV_CHUNK)
    events_scan_kernel(int64_t *__restrict__ d_total, int64_t cap, int ring, const int64_t *__restrict__ from_row,
                       const int32_t *__restrict__ ccount, const int32_t *__restrict__ clast,
                       int32_t *__restrict__ cbase, int32_t *__restrict__ cprev, EvHeader *__restrict__ hdr,
                       int64_t *__restrict__ out_n_events, int regroup, const int64_t *__restrict__ gkey,
                       const int64_t *__restrict__ gord) {
    __shared__ int s_sum[EV_CHUNK], s_last[EV_CHUNK];
    const EvSpan sp = ev_span(d_total, cap, ring, from_row);
    const int64_t n = sp.rv.n;
    if (sp.o0 >= n) {  // nothing covered: only the count is written
        if (threadIdx.x == 0) {
            hdr->n_events = 0;
            if (out_n_events) *out_n_events = 0;
        }
        return;
    }
    const int64_t cfirst = sp.o0 / EV_CHUNK, cend = (n + EV_CHUNK - 1) / EV_CHUNK;
    int64_t carry = 0;
    int carry_last = -1;
    for (int64_t cb = cfirst; cb < cend; cb += EV_CHUNK) {
        const int64_t c = cb + threadIdx.x;
        const int v = c < cend ? ccount[c] : 0;
        const int l = c < cend ? clast[c] : -1;
        const EvScan r = ev_block_scan(v, l, s_sum, s_last);
        if (c < cend) {
            cbase[c] = (int32_t)(carry + r.sum - v);
            const int before = threadIdx.x > 0 ? s_last[threadIdx.x - 1] : -1;
            cprev[c] = before > carry_last ? before : carry_last;
        }
        const int all_sum = s_sum[EV_CHUNK - 1], all_last = s_last[EV_CHUNK - 1];
        carry += all_sum;
        if (all_last > carry_last) carry_last = all_last;
    }
    if (threadIdx.x == 0) {
        hdr->n_events = carry;
        if (out_n_events) *out_n_events = carry;
        if (regroup) {
            int64_t ord_prev = -1, key_prev = 0;
            if (sp.tail) {
                const int64_t p = slot_of(sp.rv, sp.o0 - 1);
                ord_prev = gord[p];
                key_prev = gkey[p];
            }
            d_total[VM_GSTATE_GROUPS] = ord_prev + 1 + carry;
            d_total[VM_GSTATE_LAST_KEY] = carry_last >= 0 ? sp.rv.base + carry_last : key_prev;
            d_total[VM_GSTATE_OPEN] = 0;
        }
    }
}

// ---- apply -----------------------------------------------------------------------------------------------------
// REGROUP = false: out_event_of[o], out_first_rows[e] for e < max_events, and the -1 padding of [count, max_events)
// spread over the blocks.  REGROUP = true: the key (the event's first row id, or the predecessor's key while the tail's
// first row continues its event) and the ordinal of every covered row.
template <bool REGROUP>
__global__ void __launch_bounds__(EV_CHUNK)
    events_apply_kernel(const int64_t *__restrict__ d_total, int64_t cap, int ring,
                        const int64_t *__restrict__ from_row, const uint8_t *__restrict__ flags,
                        const int32_t *__restrict__ cbase, const int32_t *__restrict__ cprev,
                        const EvHeader *__restrict__ hdr, int64_t *__restrict__ out_event_of, int64_t max_events,
                        int64_t *__restrict__ out_first_rows, int64_t *__restrict__ gkey, int64_t *__restrict__ gord) {
    __shared__ int s_sum[EV_CHUNK], s_last[EV_CHUNK];
    const EvSpan sp = ev_span(d_total, cap, ring, from_row);
    const int64_t n = sp.rv.n;
    if (sp.o0 >= n) return;
    if (!REGROUP) {
        const int64_t step = (int64_t)gridDim.x * EV_CHUNK;
        for (int64_t i = hdr->n_events + (int64_t)blockIdx.x * EV_CHUNK + threadIdx.x; i < max_events; i += step)
            out_first_rows[i] = -1;
    }
    const int64_t c0 = (int64_t)blockIdx.x * EV_CHUNK;
    if (c0 >= n || c0 + EV_CHUNK <= sp.o0) return;  // block-uniform
    const int64_t o = c0 + threadIdx.x;
    const bool in = o < n && o >= sp.o0;
    const int flag = in ? flags[o] : 0;
    const EvScan r = ev_block_scan(flag, flag ? (int)o : -1, s_sum, s_last);
    if (!in) return;
    const int64_t idx = (int64_t)cbase[blockIdx.x] + r.sum;  // events opened among the covered rows up to and with o
    if (!REGROUP) {
        if (out_event_of) out_event_of[o] = idx - 1;
        if (flag && idx - 1 < max_events) out_first_rows[idx - 1] = sp.rv.base + o;
    } else {
        const int prev = cprev[blockIdx.x];
        const int first = r.last > prev ? r.last : prev;
        int64_t ord_prev = -1, key_prev = 0;
        if (sp.tail) {
            const int64_t p = slot_of(sp.rv, sp.o0 - 1);
            ord_prev = gord[p];
            key_prev = gkey[p];
        }
        const int64_t slot = slot_of(sp.rv, o);
        gkey[slot] = first >= 0 ? sp.rv.base + first : key_prev;
        gord[slot] = ord_prev + idx;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------
struct EvPlan {
    int64_t cap_pad;
    unsigned nch;
    size_t off_flags, off_cc, off_cl, off_cb, off_cp, total;
};

EvPlan events_plan(const vm_memory *m) {
    EvPlan p;
    p.cap_pad = (m->cap + EV_CHUNK - 1) / EV_CHUNK * EV_CHUNK;
    p.nch = (unsigned)(p.cap_pad / EV_CHUNK);
    size_t off = EV_HEADER_BYTES;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += vm_align_up(bytes, 256);
        return at;
    };
    p.off_flags = take((size_t)p.cap_pad);
    p.off_cc = take((size_t)p.nch * 4);
    p.off_cl = take((size_t)p.nch * 4);
    p.off_cb = take((size_t)p.nch * 4);
    p.off_cp = take((size_t)p.nch * 4);
    p.total = off;
    return p;
}

int events_check(vm_memory *m, double threshold, int64_t max_gap_ms, const void *workspace, size_t workspace_bytes,
                 const char *who) {
    vm_ctx *ctx = m->ctx;
    if (std::isnan(threshold)) return vm_fail(ctx, VM_ERR_INVALID, "%s: threshold is NaN", who);
    if (max_gap_ms >= 0 && !m->tag)
        return vm_fail(ctx, VM_ERR_INVALID, "%s: max_gap_ms needs a tagged memory (vm_memory_create_tagged)", who);
    const size_t need = events_plan(m).total;
    if (!workspace || workspace_bytes < need)
        return vm_fail(ctx, VM_ERR_NOMEM, "%s: workspace %zu < %zu", who, workspace_bytes, need);
    if ((uintptr_t)workspace & 255) return vm_fail(ctx, VM_ERR_INVALID, "%s: workspace must be 256-byte aligned", who);
    return VM_OK;
}

template <int DT>
int events_run(vm_memory *m, bool regroup, double threshold, int64_t max_gap_ms, const int64_t *from_row,
               double *out_links, int64_t *out_event_of, int64_t max_events, int64_t *out_first_rows,
               int64_t *out_n_events, char *ws, hipStream_t st) {
    vm_ctx *ctx = m->ctx;
    const EvPlan p = events_plan(m);
    EvHeader *hdr = (EvHeader *)ws;
    uint8_t *flags = (uint8_t *)(ws + p.off_flags);
    int32_t *ccount = (int32_t *)(ws + p.off_cc), *clast = (int32_t *)(ws + p.off_cl);
    int32_t *cbase = (int32_t *)(ws + p.off_cb), *cprev = (int32_t *)(ws + p.off_cp);
    vm_prof_scope prof(ctx, VM_PROF_TOPK_EXACT, st);
#ifdef VM_DEV_SWITCHES
    if (VM_DEV_ENV("EVENTS_SIMPLE", 0)) {
        events_link_kernel<DT><<<p.nch, EV_CHUNK, 0, st>>>(m->rows, m->norm64, m->tag, m->d_total, m->cap, m->ring,
                                                          m->D, from_row, threshold, max_gap_ms, out_links, flags,
                                                          ccount, clast);
    } else
#endif
    {
        auto kern = events_link_stream_kernel<DT>;
        if (int rc = vm_lds_opt_in(ctx, kern, 2 * EV_BUF, "vm_memory_events")) return rc;
        kern<<<p.nch, EV_CHUNK, 2 * EV_BUF, st>>>(m->rows, m->norm64, m->tag, m->d_total, m->cap, m->ring, m->D, from_row,
                                                 threshold, max_gap_ms, out_links, flags, ccount, clast);
    }
    VM_LAUNCH_CHECK(ctx);
    events_scan_kernel<<<1, EV_CHUNK, 0, st>>>(m->d_total, m->cap, m->ring, from_row, ccount, clast, cbase, cprev, hdr,
                                               out_n_events, regroup ? 1 : 0, m->gkey, m->gord);
    VM_LAUNCH_CHECK(ctx);
    if (regroup)
        events_apply_kernel<true><<<p.nch, EV_CHUNK, 0, st>>>(m->d_total, m->cap, m->ring, from_row, flags, cbase, cprev,
                                                             hdr, nullptr, 0, nullptr, m->gkey, m->gord);
    else if (out_event_of || max_events > 0)
        events_apply_kernel<false><<<p.nch, EV_CHUNK, 0, st>>>(m->d_total, m->cap, m->ring, nullptr, flags, cbase, cprev,
                                                              hdr, out_event_of, max_events, out_first_rows, nullptr,
                                                              nullptr);
    VM_LAUNCH_CHECK(ctx);
    return VM_OK;
}

}  // namespace

extern "C" size_t vm_memory_events_workspace_bytes(const vm_memory *m) {
    if (!m) return 0;
    return events_plan(m).total;
}

extern "C" int vm_memory_events(vm_memory *m, double threshold, int64_t max_gap_ms, double *out_links,
                                int64_t *out_event_of, int64_t max_events, int64_t *out_first_rows,
                                int64_t *out_n_events, void *workspace, size_t workspace_bytes, void *stream) {
    if (!m) return VM_ERR_INVALID;
    if (max_events < 0 || !out_n_events || (max_events > 0) != (out_first_rows != nullptr))
        return vm_fail(m->ctx, VM_ERR_INVALID, "vm_memory_events: bad arguments");
    const int rc = events_check(m, threshold, max_gap_ms, workspace, workspace_bytes, "vm_memory_events");
    if (rc != VM_OK) return rc;
    if (m->dtype == VM_F16)
        return events_run<VM_F16>(m, false, threshold, max_gap_ms, nullptr, out_links, out_event_of, max_events,
                                  out_first_rows, out_n_events, (char *)workspace, (hipStream_t)stream);
    return events_run<VM_BF16>(m, false, threshold, max_gap_ms, nullptr, out_links, out_event_of, max_events,
                               out_first_rows, out_n_events, (char *)workspace, (hipStream_t)stream);
}

extern "C" int vm_memory_regroup_events(vm_memory *m, double threshold, int64_t max_gap_ms, const int64_t *from_row,
                                        int64_t *out_n_events, void *workspace, size_t workspace_bytes, void *stream) {
    if (!m) return VM_ERR_INVALID;
    if (!m->gkey)
        return vm_fail(m->ctx, VM_ERR_INVALID, "vm_memory_regroup_events: the memory is not grouped");
    const int rc = events_check(m, threshold, max_gap_ms, workspace, workspace_bytes, "vm_memory_regroup_events");
    if (rc != VM_OK) return rc;
    if (m->dtype == VM_F16)
        return events_run<VM_F16>(m, true, threshold, max_gap_ms, from_row, nullptr, nullptr, 0, nullptr, out_n_events,
                                  (char *)workspace, (hipStream_t)stream);
    return events_run<VM_BF16>(m, true, threshold, max_gap_ms, from_row, nullptr, nullptr, 0, nullptr, out_n_events,
                               (char *)workspace, (hipStream_t)stream);
}

extern "C" const int64_t *vm_memory_group_ordinals(const vm_memory *m) { return m ? m->gord : nullptr; }
