// Sequence search: where do J <= 16 ORDERED steps occur in the memory, each step at most G <= 16 rows after the one before
// (include/vidmem.h vm_topk_cosine_seq)?  The clip search (topk_clip.hip) scores step i against row r + i
// exactly; here a CHAIN r_0 < r_1 < ... < r_{J-1} of eligible rows with 1 <= r_j - r_{j-1} <= G inside one video scores the
// mean of its J reference cosines, a row r scores A(r) = the best chain that ENDS at r - a dynamic programme over the rows,
// P_j(r) = max_{d in 1..G} P_{j-1}(r - d) + e_j(r), ties to the smallest d - and the k answers are the peaks of A.
//
// Two-stage and certified like the clip search, whose stages it runs unchanged wherever they fit (topk_clip_parts.h):
//   pack     : vm_clip_pack: each sequence -> one zero-padded 16-query tile + the exact fp64 norm of every step
//   scan     : vm_clip_scan without scopes: S[16 c + j][slot] = the fp32 score of every live row against step j
//   align    : seq_align_kernel, one block per (segment of SEQ_SEG end rows, sequence): eligibility and tag breaks of the
//              segment and of the (J-1) G rows before it into LDS, then the J layers ping-pong in LDS IN FP64 over
//              e~_j = (double)S / ||q_j||, Bf[c][slot(r)] = (float)(P~_{J-1}(r) / J), -inf when r is no END.  A maximum
//              moves no more than its most-moved argument, so layer j lies within (j + 1) cert_eps(D) of the exact one
//              and |Bf - A| <= eps_seq = cert_eps(D) + 2^-23 = the clip search's eps_w
//   peaks    : vm_clip_peaks, select: vm_key_image_select, as in the clip search
//   re-score : seq_cone_kernel, one block per (candidate, sequence): the exact e_j on the candidate's cone - the rows
//              that can lie on a chain ending at the candidate or at a competitor, at most (J-1) G + 2 min_sep - 1 = 303 -
//              then the exact layers in LDS and the exact peak test
//   rank     : vm_clip_rank: the exact peaks among the best M ranked, filtered, written; the certificate; the flags
//   redo     : flagged sequences: J launches of seq_redo_layer_kernel, exact fp64 layers over ALL rows in two arrays of
//              8 x capacity bytes per sequence, e_j computed on the fly; then vm_clip_redo_slices and vm_topk_redo_merge
//   trace    : seq_cone_kernel again, one block per (hit, sequence) over the rows just written: the exact layers on the
//              hit's cone with the step d each cell took, followed back from the end -> out_step_rows, out_step_scores
// Every launch reads the row count, the steps and the masks from the device and sizes its grid from the capacity: capturable.
#include "topk_clip_parts.h"

#include <cmath>

namespace {

constexpr int SEQ_JMAX = CLIP_LMAX;  // steps per sequence = queries per scan tile
constexpr int SEQ_GMAX = 16;         // max_step
constexpr int SEQ_HALO = (SEQ_JMAX - 1) * SEQ_GMAX;          // rows before an end row that its chains can reach: 240
constexpr int SEQ_SEG = 768;                                 // end rows per block of the align kernel
constexpr int SEQ_LOCAL = SEQ_SEG + SEQ_HALO;                // rows in LDS per block of the align kernel
constexpr int SEQ_CONE = SEQ_HALO + 2 * CLIP_SEPMAX - 1;     // rows of a candidate's cone: 303
constexpr int SQ_THREADS = 256;

struct RowState {  // per row of a block's stretch: bit 0 = eligible, bit 1 = tag break against the row before
    enum { ELIGIBLE = 1, BREAK = 2 };
};

// the state of the row of age order o (any integer): rows outside the live ones are not eligible
__device__ __forceinline__ uint8_t seq_row_state(const RingView &rv, const int64_t *__restrict__ tag,
                                                 const uint32_t *__restrict__ words, int64_t moff, bool masked,
                                                 int64_t max_gap_ms, int64_t o) {
    if (o < 0 || o >= rv.n) return 0;
    const int64_t p = slot_of(rv, o);
    uint8_t s = (!masked || mask_selects(words, moff, p)) ? RowState::ELIGIBLE : 0;
    if (tag && o > 0 && clip_tag_break(tag[slot_of(rv, o - 1)], tag[p], max_gap_ms)) s |= RowState::BREAK;
    return s;
}

// The best predecessor of local row i in `prev` (-inf = none): the largest value among i - 1 .. i - G that no tag break
// separates from i, ties to the smallest d.  -> d, 0 when there is none.
__device__ __forceinline__ int seq_best_pred(const double *prev, const uint8_t *st, int i, int G, double &best) {
    best = -INFINITY;
    int bd = 0;
    for (int d = 1; d <= G && d <= i; ++d) {
        if (st[i - d + 1] & RowState::BREAK) break;  // a break on any row in (i - d, i] ends every longer step too
        const double v = prev[i - d];
        if (v > best) {
            best = v;
            bd = d;
        }
    }
    return bd;
}

// ---- align ---------------------------------------------------------------------------------------------------
// grid (ceil(cap / SEQ_SEG), C): block (b, c) = the end rows of age order b SEQ_SEG .. of sequence c
__global__ void __launch_bounds__(SQ_THREADS)
    seq_align_kernel(const int64_t *__restrict__ d_total, int64_t cap, int ring, const int64_t *__restrict__ tag,
                     const MaskSel ms, int masked, int64_t max_gap_ms, int J, int G, const float *__restrict__ S,
                     int64_t fstride, const double *__restrict__ qn, float *__restrict__ Bf) {
    __shared__ double lay[2][SEQ_LOCAL];
    __shared__ uint8_t st[SEQ_LOCAL];
    const int c = blockIdx.y, tid = threadIdx.x;
    const RingView rv = ring_view(*d_total, cap, ring);
    const int64_t o0 = (int64_t)blockIdx.x * SEQ_SEG;
    if (o0 >= rv.n) return;  // uniform
    const int halo = (J - 1) * G;
    const int64_t left = rv.n - o0;
    const int nl = halo + (int)(left < SEQ_SEG ? left : SEQ_SEG);  // local row i = age order o0 - halo + i
    const int64_t moff = masked ? mask_offset(ms, c) : 0;
    for (int i = tid; i < nl; i += SQ_THREADS)
        st[i] = seq_row_state(rv, tag, ms.words, moff, masked != 0, max_gap_ms, o0 - halo + i);
    __syncthreads();
    for (int j = 0; j < J; ++j) {
        const double q = qn[c * SEQ_JMAX + j];
        const float *Sj = S + ((size_t)c * SEQ_JMAX + j) * fstride;
        double *cur = lay[j & 1];
        const double *prev = lay[(j & 1) ^ 1];
        for (int i = tid; i < nl; i += SQ_THREADS) {
            double v = -INFINITY;
            if (st[i] & RowState::ELIGIBLE) {
                double best = 0.0;
                if (j == 0 || seq_best_pred(prev, st, i, G, best)) {
                    const float s = Sj[slot_of(rv, o0 - halo + i)];
                    v = __dadd_rn(best, q == 0.0 ? 0.0 : __ddiv_rn((double)s, q));  // a zero step: an exact 0
                }
            }
            cur[i] = v;
        }
        __syncthreads();
    }
    const double *last = lay[(J - 1) & 1];
    for (int i = halo + tid; i < nl; i += SQ_THREADS) {
        const double v = last[i];
        Bf[(size_t)c * fstride + slot_of(rv, o0 - halo + i)] = v == -INFINITY ? -INFINITY : (float)__ddiv_rn(v, (double)J);
    }
}

// ---- the cone: re-score and trace ------------------------------------------------------------------------------
// The exact layers on the rows that decide one end row and its competitors.  Local row i = age order o - mid - halo + i,
// nl = halo + 2 mid + 1 of them; the cells whose chains could start before local row 0 (i < j G in layer j) may be short of
// a predecessor, and no chain from them reaches a local row >= halo in the last layer, so every A at or past halo and every
// step on its best chain is the exhaustive one.
//   trace == 0, grid (M + 1, C): block (x, c) = candidate x of sequence c, mid = min_sep - 1: its exact A and whether it
//                ranks before every competitor -> cand_w, cand_p
//   trace == 1, grid (k, C): block (x, c) = hit x of sequence c as out_rows holds it, mid = 0: the chain followed back
//                from the end -> out_step_rows / out_step_scores [C][k][J] (either may be null), -1 / 0.0 for a padded hit
template <int DT>
__global__ void __launch_bounds__(SQ_THREADS)
    seq_cone_kernel(const uint16_t *__restrict__ mem, const double *__restrict__ norm64, const uint16_t *__restrict__ qt,
                    const double *__restrict__ qn, const int64_t *__restrict__ d_total, int64_t cap, int ring, int D,
                    const int64_t *__restrict__ tag, const MaskSel ms, int masked, int64_t max_gap_ms, int J, int G,
                    int min_sep, int trace, const int *__restrict__ cand_o, const int *__restrict__ cand_n,
                    double *__restrict__ cand_w, int *__restrict__ cand_p, int k, const int64_t *__restrict__ out_rows,
                    int64_t *__restrict__ out_step_rows, double *__restrict__ out_step_scores) {
    __shared__ double E[SEQ_JMAX][SEQ_CONE + 1];
    __shared__ double lay[2][SEQ_CONE + 1];
    __shared__ uint8_t pred[SEQ_JMAX][SEQ_CONE + 1];
    __shared__ uint8_t st[SEQ_CONE + 1];
    __shared__ int beaten;
    const int x = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const RingView rv = ring_view(*d_total, cap, ring);
    int64_t o;
    if (trace) {
        const int64_t row = out_rows[(size_t)c * k + x];
        if (row < 0) {  // uniform: a padded hit
            for (int j = tid; j < J; j += SQ_THREADS) {
                if (out_step_rows) out_step_rows[((size_t)c * k + x) * J + j] = -1;
                if (out_step_scores) out_step_scores[((size_t)c * k + x) * J + j] = 0.0;
            }
            return;
        }
        o = row - rv.base;
    } else {
        if (x >= cand_n[c]) return;  // uniform; also an overflowed list (-1)
        o = cand_o[(size_t)c * SCMAX + x];
    }
    const int mid = trace ? 0 : min_sep - 1, halo = (J - 1) * G;
    const int nl = halo + 2 * mid + 1, ic = halo + mid;
    const int64_t ofirst = o - ic;
    const int64_t moff = masked ? mask_offset(ms, c) : 0;
    for (int i = tid; i < nl; i += SQ_THREADS)
        st[i] = seq_row_state(rv, tag, ms.words, moff, masked != 0, max_gap_ms, ofirst + i);
    if (tid == 0) beaten = 0;
    __syncthreads();
    for (int t = tid; t < J * nl; t += SQ_THREADS) {
        const int j = t / nl, i = t - j * nl;
        if (!(st[i] & RowState::ELIGIBLE)) continue;
        const int64_t p = slot_of(rv, ofirst + i);
        const int q = c * SEQ_JMAX + j;
        E[j][i] = ref_cosine(ref_dot<DT>(qt + (size_t)q * D, mem + (size_t)p * D, D), qn[q], norm64[p]);
    }
    __syncthreads();
    for (int j = 0; j < J; ++j) {
        double *cur = lay[j & 1];
        const double *prev = lay[(j & 1) ^ 1];
        for (int i = tid; i < nl; i += SQ_THREADS) {
            double v = -INFINITY;
            int d = 0;
            if (st[i] & RowState::ELIGIBLE) {
                double best = 0.0;
                if (j == 0 || (d = seq_best_pred(prev, st, i, G, best)) != 0) v = __dadd_rn(best, E[j][i]);
            }
            cur[i] = v;
            pred[j][i] = (uint8_t)d;
        }
        __syncthreads();
    }
    const double *last = lay[(J - 1) & 1];
    if (trace) {
        if (tid == 0) {
            int r = ic;
            for (int j = J - 1; j >= 0; --j) {
                if (out_step_rows) out_step_rows[((size_t)c * k + x) * J + j] = rv.base + ofirst + r;
                if (out_step_scores) out_step_scores[((size_t)c * k + x) * J + j] = E[j][r];
                r -= pred[j][r];
            }
        }
        return;
    }
    const double a0 = __ddiv_rn(last[ic], (double)J);
    for (int i = halo + tid; i < nl; i += SQ_THREADS) {  // ranks before the candidate: higher A, or the same A and a lower end
        if (i == ic || last[i] == -INFINITY) continue;
        const double a2 = __ddiv_rn(last[i], (double)J);
        if (a2 > a0 || (a2 == a0 && i < ic)) beaten = 1;
    }
    __syncthreads();
    if (tid == 0) {
        cand_w[(size_t)c * SCMAX + x] = a0;
        cand_p[(size_t)c * SCMAX + x] = beaten ? 0 : 1;
    }
}

// ---- redo ------------------------------------------------------------------------------------------------------
// grid (ceil(cap / SQ_THREADS), C), thread = the row of age order o of a flagged sequence: layer j from layer j - 1, both
// [C][fstride] fp64 indexed by age order, -inf = the cell does not exist.  The last layer is written divided by J: A.
template <int DT>
__global__ void __launch_bounds__(SQ_THREADS)
    seq_redo_layer_kernel(const uint16_t *__restrict__ mem, const double *__restrict__ norm64,
                          const uint16_t *__restrict__ qt, const double *__restrict__ qn,
                          const int64_t *__restrict__ d_total, int64_t cap, int ring, int D,
                          const int64_t *__restrict__ tag, const MaskSel ms, int masked, int64_t max_gap_ms, int J, int G,
                          int j, const int32_t *__restrict__ flags, int64_t fstride, const double *__restrict__ prev,
                          double *__restrict__ cur) {
    const int c = blockIdx.y;
    if (flags[c] == 0) return;  // uniform
    const RingView rv = ring_view(*d_total, cap, ring);
    const int64_t o = (int64_t)blockIdx.x * SQ_THREADS + threadIdx.x;
    if (o >= rv.n) return;
    const int64_t p = slot_of(rv, o);
    const int64_t moff = masked ? mask_offset(ms, c) : 0;
    double v = -INFINITY;
    if (!masked || mask_selects(ms.words, moff, p)) {
        double best = 0.0;
        bool found = j == 0;
        if (j > 0) {
            best = -INFINITY;
            const double *pc = prev + (size_t)c * fstride;
            int64_t tc = tag ? tag[p] : 0;
            for (int d = 1; d <= G && d <= o; ++d) {
                if (tag) {  // a break on any row in (o - d, o] ends every longer step too
                    const int64_t tp = tag[slot_of(rv, o - d)];
                    if (clip_tag_break(tp, tc, max_gap_ms)) break;
                    tc = tp;
                }
                const double pv = pc[o - d];
                if (pv > best) best = pv;
            }
            found = best != -INFINITY;
        }
        if (found) {
            const int q = c * SEQ_JMAX + j;
            const double e = ref_cosine(ref_dot<DT>(qt + (size_t)q * D, mem + (size_t)p * D, D), qn[q], norm64[p]);
            v = __dadd_rn(best, e);
            if (j == J - 1) v = __ddiv_rn(v, (double)J);
        }
    }
    cur[(size_t)c * fstride + o] = v;
}

// ---- host --------------------------------------------------------------------------------------------------
struct QPlan : SelectPlan {  // the select stage's arrays are its base's
    size_t off_qt, off_qn, off_S, off_bf, off_key, off_cw, off_cp, off_flags, off_lay, off_ps, off_po, total;
};

QPlan seq_plan(const vm_memory *m, int C, int k) {
    QPlan p;
    static_cast<TopkGeom &>(p) = vm_topk_geom(m, C * SEQ_JMAX, k, TS_THREADS, VM_REDO_CHUNK_SCOPED);
    p.fstride = (m->cap + 63) / 64 * 64;  // the columns' padding: a tail tile writes its 16 scores
    WsBump ws;
    p.off_qt = ws.take((size_t)C * SEQ_JMAX * m->D * 2);
    p.off_qn = ws.take((size_t)C * SEQ_JMAX * 8);
    p.off_S = ws.take((size_t)C * SEQ_JMAX * (size_t)p.fstride * 4);
    p.off_bf = ws.take((size_t)C * (size_t)p.fstride * 4);
    p.off_key = ws.take((size_t)C * (size_t)p.fstride * 4);
    p.off_co = ws.take((size_t)C * SCMAX * 4);
    p.off_ck = ws.take((size_t)C * SCMAX * 4);
    p.off_cn = ws.take((size_t)C * 4);
    p.off_cw = ws.take((size_t)C * SCMAX * 8);
    p.off_cp = ws.take((size_t)C * SCMAX * 4);
    p.off_flags = ws.take((size_t)C * 4);
    p.off_cut = ws.take((size_t)C * 4);
    p.off_cc = ws.take((size_t)C * 4);
    p.off_cbuf = ws.take((size_t)C * SEL_CAP * 8);
    p.off_lay = ws.take(2 * (size_t)C * (size_t)p.fstride * 8);  // the redo's two exact layers
    p.off_ps = ws.take((size_t)p.nblk * C * k * 8);
    p.off_po = ws.take((size_t)p.nblk * C * k * 8);
    p.total = ws.off;
    return p;
}

bool seq_shape_ok(int C, int J, int k) { return C >= 1 && J >= 1 && J <= SEQ_JMAX && k >= 1 && k <= SKMAX; }

struct SeqCall {
    const void *steps;
    int C, J, k, G, min_sep;
    int64_t max_gap_ms;
    MaskSel ms;
    int masked;
    int use_min;
    double min_score;
    int score_mode;
    double *out_scores;
    int64_t *out_rows, *out_step_rows;
    double *out_step_scores;
};

int seq_check(vm_memory *m, const void *steps, int C, int J, int k, int G, int min_sep, int64_t max_gap_ms,
              const uint32_t *masks, int n_masks, const int32_t *mask_index, int use_min, double min_score,
              int score_mode, const double *out_scores, const int64_t *out_rows, const void *workspace,
              size_t workspace_bytes, const char *who) {
    vm_ctx *ctx = m->ctx;
    if (!steps || !out_scores || !out_rows || C < 1) return vm_fail(ctx, VM_ERR_INVALID, "%s: bad arguments", who);
    if (J < 1 || J > SEQ_JMAX) return vm_fail(ctx, VM_ERR_INVALID, "%s: J=%d outside [1, %d]", who, J, SEQ_JMAX);
    if (G < 1 || G > SEQ_GMAX)
        return vm_fail(ctx, VM_ERR_INVALID, "%s: max_step=%d outside [1, %d]", who, G, SEQ_GMAX);
    if (k < 1 || k > SKMAX) return vm_fail(ctx, VM_ERR_INVALID, "%s: k=%d outside [1, %d]", who, k, SKMAX);
    if (min_sep < 1 || min_sep > CLIP_SEPMAX)
        return vm_fail(ctx, VM_ERR_INVALID, "%s: min_sep=%d outside [1, %d]", who, min_sep, CLIP_SEPMAX);
    if (max_gap_ms >= 0 && !m->tag)
        return vm_fail(ctx, VM_ERR_INVALID, "%s: max_gap_ms needs a tagged memory (vm_memory_create_tagged)", who);
    if (use_min && std::isnan(min_score)) return vm_fail(ctx, VM_ERR_INVALID, "%s: min_score is NaN", who);
    if (int rc = vm_check_score_mode(ctx, score_mode)) return rc;
    if (masks)  // one mask per sequence
        if (int rc = mask_operand_check(m, masks, n_masks, mask_index, C, who)) return rc;
    const size_t need = seq_plan(m, C, k).total;
    if (!workspace || workspace_bytes < need)
        return vm_fail(ctx, VM_ERR_NOMEM, "%s: workspace %zu < %zu", who, workspace_bytes, need);
    if (((uintptr_t)workspace & 255) || ((uintptr_t)steps & 15))
        return vm_fail(ctx, VM_ERR_INVALID, "%s: workspace must be 256-byte and steps 16-byte aligned", who);
    return VM_OK;
}

template <int DT>
int seq_cone(vm_memory *m, const QPlan &p, const SeqCall &a, char *ws, int trace, hipStream_t st) {
    seq_cone_kernel<DT><<<dim3(trace ? a.k : p.M + 1, a.C), SQ_THREADS, 0, st>>>(
        m->rows, m->norm64, (const uint16_t *)(ws + p.off_qt), (const double *)(ws + p.off_qn), m->d_total, m->cap,
        m->ring, m->D, m->tag, a.ms, a.masked, a.max_gap_ms, a.J, a.G, a.min_sep, trace, (const int *)(ws + p.off_co),
        (const int *)(ws + p.off_cn), (double *)(ws + p.off_cw), (int *)(ws + p.off_cp), a.k, a.out_rows,
        a.out_step_rows, a.out_step_scores);
    VM_LAUNCH_CHECK(m->ctx);
    return VM_OK;
}

// the flagged sequences exhaustively, then the chains of every sequence's hits
template <int DT>
int seq_redo(vm_memory *m, const QPlan &p, const SeqCall &a, char *ws, hipStream_t st) {
    vm_ctx *ctx = m->ctx;
    vm_prof_scope prof(ctx, VM_PROF_TOPK_EXACT, st);
    const int32_t *flags = (const int32_t *)(ws + p.off_flags);
    double *lay[2] = {(double *)(ws + p.off_lay), (double *)(ws + p.off_lay) + (size_t)a.C * (size_t)p.fstride};
    double *part_s = (double *)(ws + p.off_ps);
    int64_t *part_o = (int64_t *)(ws + p.off_po);
    const dim3 grid((unsigned)((m->cap + SQ_THREADS - 1) / SQ_THREADS), a.C);
    for (int j = 0; j < a.J; ++j) {
        seq_redo_layer_kernel<DT><<<grid, SQ_THREADS, 0, st>>>(
            m->rows, m->norm64, (const uint16_t *)(ws + p.off_qt), (const double *)(ws + p.off_qn), m->d_total, m->cap,
            m->ring, m->D, m->tag, a.ms, a.masked, a.max_gap_ms, a.J, a.G, j, flags, p.fstride, lay[(j & 1) ^ 1],
            lay[j & 1]);
        VM_LAUNCH_CHECK(ctx);
    }
    if (int rc = vm_clip_redo_slices(m, p.nblk, a.C, a.k, a.min_sep, flags, p.fstride, lay[(a.J - 1) & 1], part_s, part_o,
                                     st))
        return rc;
    if (int rc = vm_topk_redo_merge(m, part_s, part_o, p.nblk, a.C, a.k, flags, a.use_min, a.min_score, a.score_mode, 1,
                                    0, a.out_scores, a.out_rows, nullptr, nullptr, st))
        return rc;
    if (!a.out_step_rows && !a.out_step_scores) return VM_OK;
    return seq_cone<DT>(m, p, a, ws, 1, st);
}

template <int DT>
int seq_topk(vm_memory *m, const SeqCall &a, int32_t *out_uncertified, int32_t *out_query_flags, char *ws,
             hipStream_t st) {
    vm_ctx *ctx = m->ctx;
    const QPlan p = seq_plan(m, a.C, a.k);
    uint16_t *qt = (uint16_t *)(ws + p.off_qt);
    double *qn = (double *)(ws + p.off_qn);
    float *S = (float *)(ws + p.off_S);
    float *Bf = (float *)(ws + p.off_bf);
    uint32_t *key = (uint32_t *)(ws + p.off_key);
    {
        vm_prof_scope prof(ctx, VM_PROF_TOPK_SCAN, st);
        if (int rc = vm_clip_pack(m, a.steps, a.C, a.J, qt, qn, st)) return rc;
        if (int rc = vm_clip_scan(m, p, qt, a.C, nullptr, nullptr, p.fstride, S, st)) return rc;
    }
    // developer probe (tools/seq_probe.py, the developer library only): 1 = return after the scan, 2 = after the align
    // kernel, so that event-timed calls give each stage's time by difference; the outputs are then not written
    const long stop = VM_DEV_ENV("SEQ_STOP", 0);
    if (stop == 1) return VM_OK;
    {
        vm_prof_scope prof(ctx, VM_PROF_TOPK_FINALIZE, st);
        const dim3 agrid((unsigned)((m->cap + SEQ_SEG - 1) / SEQ_SEG), a.C);
        seq_align_kernel<<<agrid, SQ_THREADS, 0, st>>>(m->d_total, m->cap, m->ring, m->tag, a.ms, a.masked, a.max_gap_ms,
                                                      a.J, a.G, S, p.fstride, qn, Bf);
        VM_LAUNCH_CHECK(ctx);
        if (stop == 2) return VM_OK;
        if (int rc = vm_clip_peaks(m, a.C, a.min_sep, Bf, p.fstride, key, st)) return rc;
        if (int rc = vm_key_image_select(m, p, key, a.C, ws, st)) return rc;
        if (int rc = seq_cone<DT>(m, p, a, ws, 0, st)) return rc;
        if (int rc = vm_clip_rank(m, a.C, a.J, qn, (const int *)(ws + p.off_co), (const uint32_t *)(ws + p.off_ck),
                                  (const int *)(ws + p.off_cn), (const double *)(ws + p.off_cw),
                                  (const int *)(ws + p.off_cp), p.M, a.k, a.use_min, a.min_score, a.score_mode,
                                  a.out_scores, a.out_rows, out_uncertified, (int32_t *)(ws + p.off_flags),
                                  out_query_flags, st))
            return rc;
    }
    return seq_redo<DT>(m, p, a, ws, st);
}

template <int DT>
int seq_exact(vm_memory *m, const SeqCall &a, char *ws, hipStream_t st) {
    const QPlan p = seq_plan(m, a.C, a.k);
    if (int rc = vm_clip_pack(m, a.steps, a.C, a.J, (uint16_t *)(ws + p.off_qt), (double *)(ws + p.off_qn), st))
        return rc;
    if (int rc = vm_fill_flags(m, (int32_t *)(ws + p.off_flags), a.C, st)) return rc;
    return seq_redo<DT>(m, p, a, ws, st);
}

int seq_entry(vm_memory *m, const void *steps, int C, int J, int k, int max_step, int min_sep, int64_t max_gap_ms,
              const uint32_t *masks, int n_masks, const int32_t *mask_index, int use_min_score, double min_score,
              int score_mode, double *out_scores, int64_t *out_rows, int64_t *out_step_rows, double *out_step_scores,
              int32_t *out_uncertified, int32_t *out_query_flags, void *workspace, size_t workspace_bytes, void *stream,
              bool exact, const char *who) {
    if (!m) return VM_ERR_INVALID;
    const int rc = seq_check(m, steps, C, J, k, max_step, min_sep, max_gap_ms, masks, n_masks, mask_index, use_min_score,
                             min_score, score_mode, out_scores, out_rows, workspace, workspace_bytes, who);
    if (rc != VM_OK) return rc;
    const SeqCall a = {steps,      C,
                       J,          k,
                       max_step,   min_sep,
                       max_gap_ms, {masks, mask_index, n_masks, mask_words(m)},
                       masks ? 1 : 0, use_min_score,
                       min_score,  score_mode,
                       out_scores, out_rows,
                       out_step_rows, out_step_scores};
    return vm_by_dtype(m, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (exact) return seq_exact<DT>(m, a, (char *)workspace, (hipStream_t)stream);
        return seq_topk<DT>(m, a, out_uncertified, out_query_flags, (char *)workspace, (hipStream_t)stream);
    });
}

}  // namespace

extern "C" size_t vm_topk_seq_workspace_bytes(const vm_memory *m, int C, int J, int k) {
    if (!m || !seq_shape_ok(C, J, k)) return 0;
    return seq_plan(m, C, k).total;
}

extern "C" int vm_topk_cosine_seq(vm_memory *m, const void *steps, int C, int J, int k, int max_step, int min_sep,
                                  int64_t max_gap_ms, const uint32_t *masks, int n_masks, const int32_t *mask_index,
                                  int use_min_score, double min_score, int score_mode, double *out_scores,
                                  int64_t *out_rows, int64_t *out_step_rows, double *out_step_scores,
                                  int32_t *out_uncertified, int32_t *out_query_flags, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    return seq_entry(m, steps, C, J, k, max_step, min_sep, max_gap_ms, masks, n_masks, mask_index, use_min_score, min_score,
                     score_mode, out_scores, out_rows, out_step_rows, out_step_scores, out_uncertified, out_query_flags,
                     workspace, workspace_bytes, stream, false, "vm_topk_cosine_seq");
}

extern "C" int vm_topk_cosine_seq_exact(vm_memory *m, const void *steps, int C, int J, int k, int max_step, int min_sep,
                                        int64_t max_gap_ms, const uint32_t *masks, int n_masks,
                                        const int32_t *mask_index, int use_min_score, double min_score, int score_mode,
                                        double *out_scores, int64_t *out_rows, int64_t *out_step_rows,
                                        double *out_step_scores, void *workspace, size_t workspace_bytes, void *stream) {
    return seq_entry(m, steps, C, J, k, max_step, min_sep, max_gap_ms, masks, n_masks, mask_index, use_min_score, min_score,
                     score_mode, out_scores, out_rows, out_step_rows, out_step_scores, nullptr, nullptr, workspace,
                     workspace_bytes, stream, true, "vm_topk_cosine_seq_exact");
}
