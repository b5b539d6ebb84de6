// Test-only C entry points over the encoder's internal kernel launchers (csrc/vm_kernels.h).  Host code alone: no kernel
// and no arithmetic lives here.  Built as libvidmem_stages.so and linked against the release libvidmem.so (rpath
// $ORIGIN), so the stage tests run the very object code that ships; the release library itself exports nothing new.
#include "../../real-time-brain-inspired-video-memory_amd/csrc/vm_kernels.h"

void vm_gemm_set_variant(int v);  // gemm.hip (as tools/gemm_bench.hip declares it)

extern "C" {

int vmt_gemm(vm_ctx *ctx, int dtype, int epi, const uint16_t *X, const uint16_t *W, const float *bias, uint16_t *out16,
             float *out32, const float *pos, int M, int N, int K, int ldx, int ldo, int P, int T, int prof_cat,
             int head_major, int hm_rows, int hm_stride, hipStream_t st) {
    GemmArgs g{};
    g.X = X;
    g.W = W;
    g.bias = bias;
    g.out16 = out16;
    g.out32 = out32;
    g.pos = pos;
    g.M = M;
    g.N = N;
    g.K = K;
    g.ldx = ldx;
    g.ldo = ldo;
    g.P = P;
    g.T = T;
    g.prof_cat = prof_cat;
    g.head_major = head_major;
    g.hm_rows = hm_rows;
    g.hm_stride = hm_stride;
    return vm_gemm(ctx, dtype, g, epi, st);
}

void vmt_gemm_set_variant(int v) { vm_gemm_set_variant(v); }

int vmt_attention(vm_ctx *ctx, int dtype, const uint16_t *qkv, uint16_t *ctx_out, int B, int T, int heads, int q_rows,
                  int causal, hipStream_t st) {
    return vm_attention(ctx, dtype, qkv, ctx_out, B, T, heads, st, q_rows, causal);
}

int vmt_resid_layernorm(vm_ctx *ctx, int dtype, float *x32, const uint16_t *delta16, const uint16_t *deltaB16,
                        int write_x, const float *gamma, const float *beta, float eps, uint16_t *out16, int rows, int H,
                        int rstride, int lowreg, hipStream_t st) {
    return vm_resid_layernorm(ctx, dtype, x32, delta16, deltaB16, write_x, gamma, beta, eps, out16, rows, H, st, rstride,
                              lowreg);
}

int vmt_embed(vm_ctx *ctx, int dtype, const uint16_t *patch16, const float *cls, const float *pos, const float *pre_g,
              const float *pre_b, float eps, int pre_ln, float *x32, int B, int T, int H, hipStream_t st) {
    return vm_embed(ctx, dtype, patch16, cls, pos, pre_g, pre_b, eps, pre_ln, x32, B, T, H, st);
}

int vmt_pool(vm_ctx *ctx, int dtype, const float *x, const uint16_t *delta16, const uint16_t *deltaB16,
             const float *gamma, const float *beta, float eps, const uint16_t *proj_w, int proj_dim, int l2, uint16_t *out,
             int B, int T, int H, const int32_t *pool_row, hipStream_t st) {
    return vm_pool(ctx, dtype, x, delta16, deltaB16, gamma, beta, eps, proj_w, proj_dim, l2, out, B, T, H, st, pool_row);
}

int vmt_text_embed(vm_ctx *ctx, const int32_t *ids, const float *tok, const float *pos, int vocab, int eot_id,
                   float *x32, int32_t *pool_row, int32_t *flags, int B, int T, int H, hipStream_t st) {
    return vm_text_embed(ctx, ids, tok, pos, vocab, eot_id, x32, pool_row, flags, B, T, H, st);
}

}  // extern "C"
