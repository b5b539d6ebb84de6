// The stages of the clip search (topk_clip.hip) that the sequence search (topk_seq.hip) runs
// unchanged: the pack of up to 16 vectors per clip into one query tile, the ClipScan tile scan without scopes, the
// possible-peak filter over one fp32 score per (clip, slot), the rank-and-certify kernel over the re-scored candidates and
// the redo's peak test with the stable top-k per slice.  The kernels are compiled once, in topk_clip.hip;
// here are the constants and the launchers another unit calls.  What "score of slot p" means is the caller's: the clip
// search keys a window by its START row, the sequence search a chain by its END row; nothing below depends on it.
#pragma once
#include "topk_scope_select.h"

#include <climits>

constexpr int CLIP_LMAX = 16;    // frames per clip = queries per scan tile
constexpr int CLIP_SEPMAX = 32;  // min_sep
constexpr int64_t CLIP_MS_MASK = ((int64_t)1 << 40) - 1;  // a tag = source << 40 | milliseconds

// the tag part of vm_memory_events' opening rule (events.hip ev_opens) between a row and its successor
__device__ __forceinline__ bool clip_tag_break(int64_t tp, int64_t tc, int64_t max_gap_ms) {
    const bool up = tp == LLONG_MIN, uc = tc == LLONG_MIN;
    if (up != uc) return true;
    if (up) return false;
    const int64_t step = (tc & CLIP_MS_MASK) - (tp & CLIP_MS_MASK);
    return (tp >> 40) != (tc >> 40) || (max_gap_ms >= 0 && (step < 0 || step > max_gap_ms));
}

// vectors [C, L, D] -> qt [C][16][D] (zeros past L) and qn [C][16], the exact fp64 norm of every vector
int vm_clip_pack(vm_memory *m, const void *vectors, int C, int L, uint16_t *qt, double *qn, hipStream_t st);
// S[16 c + i][slot] = the fp32 score of every live row against vector i of clip c; scope_lo / scope_hi per clip or null
int vm_clip_scan(vm_memory *m, const ScanGeom &g, const uint16_t *qt, int C, const int64_t *scope_lo,
                 const int64_t *scope_hi, int64_t fstride, float *S, hipStream_t st);
// key[c][slot(o)] = okey32(Bf) unless Bf is -inf or a competitor within min_sep exceeds it by more than 2 eps_w, else 0
int vm_clip_peaks(vm_memory *m, int C, int min_sep, const float *Bf, int64_t fstride, uint32_t *key, hipStream_t st);
// the exact peaks among the best M re-scored candidates ranked, filtered and written; the certificate; the flags
int vm_clip_rank(vm_memory *m, int C, int L, const double *qn, const int *cand_o, const uint32_t *cand_k,
                 const int *cand_n, const double *cand_w, const int *cand_p, int M, int k, int use_min, double min_score,
                 int score_mode, double *out_scores, int64_t *out_rows, int32_t *uncertified, int32_t *flags,
                 int32_t *user_flags, hipStream_t st);
// flagged clips: the exact peak test on W64[c][age order] (-inf = none) and the stable top-k of peaks per slice
int vm_clip_redo_slices(vm_memory *m, int nblk, int C, int k, int min_sep, const int32_t *flags, int64_t fstride,
                        const double *W64, double *part_s, int64_t *part_o, hipStream_t st);
