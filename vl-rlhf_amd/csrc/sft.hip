// Supervised fine-tuning on the fused lm-head (gfx950): the batch-mean cross-entropy of the label rows and the row-blocked drive of
// the lm-head backward.  The heavy kernels are the DPO path's own (vlr_lmhead_logps_fwd / _bwd, vlr_gemm_bf16): what is new is the
// reduction of the per-row log-probabilities to ONE scalar over the whole batch (nn.CrossEntropyLoss(), reference
// Llava/__init__.py:246-257) and a walk over the rows that keeps d logits [row_block][V] instead of [R][V] in HBM.
#include <stdlib.h>

#include "../../include/vlr.h"
#include "common.h"

// ------------------------------------------------------------------------------------------------------------
// loss = -(1/R) sum_r tok_logp[r].  Two stages in a fixed order, no atomics (as vlr_grad_sqnorm): block b sums the elements
// b*256 + t + k * (P*256) - P depends on R only - and one workgroup folds the P partials.  Two calls give the same bits.
// out3 = {loss, R, -1/R}: the count for cross-rank weighting, -1/R = d loss / d tok_logp[r] for vlr_lmhead_ce_bwd.
// ------------------------------------------------------------------------------------------------------------
#define VLR_CE_BLOCKS 256
__global__ __launch_bounds__(256) void ce_partial_kernel(const float* __restrict__ tok, int R, float* __restrict__ part) {
    __shared__ float red[16];
    float s = 0.f;
    const int step = gridDim.x * 256;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < R; i += step) s += tok[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void ce_final_kernel(const float* __restrict__ part, int P, int R, float* __restrict__ out) {
    __shared__ float red[16];
    float s = 0.f;
    for (int i = threadIdx.x; i < P; i += 256) s += part[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
        out[0] = -s / (float)R;
        out[1] = (float)R;
        out[2] = -1.f / (float)R;
    }
}

extern "C" int vlr_ce_mean_workspace_bytes(void) { return VLR_CE_BLOCKS * 4; }
extern "C" int vlr_ce_mean_fwd(const float* tok_logp, int R, void* workspace, float* out3, hipStream_t st) {
    VLR_REQUIRE(tok_logp && workspace && out3, "vlr_ce_mean_fwd: null operand");
    VLR_REQUIRE(R > 0, "vlr_ce_mean_fwd: R=%d rows (an empty selection has no mean)", R);
    const int P = R < VLR_CE_BLOCKS * 256 ? (R + 255) / 256 : VLR_CE_BLOCKS;
    hipLaunchKernelGGL(ce_partial_kernel, dim3(P), dim3(256), 0, st, tok_logp, R, (float*)workspace);
    hipLaunchKernelGGL(ce_final_kernel, dim3(1), dim3(256), 0, st, (const float*)workspace, P, R, out3);
    return vlr_check_launch("vlr_ce_mean_fwd");
}

// ------------------------------------------------------------------------------------------------------------
// Row-blocked lm-head backward of the cross-entropy.  Default block: the largest multiple of 256 rows (the GEMM's row tile) whose
// d logits bf16 [rb][V], fp32 logits [rb][V] (shapes the fused kernel does not take) and lm-head partials stay under 1 GiB.
// ------------------------------------------------------------------------------------------------------------
extern "C" int vlr_lmhead_ce_row_block(int R, int V, int H) {
    if (R <= 0 || V <= 0) return 0;
    const long budget = 1L << 30;
    const long per_row = (long)V * 6 + vlr_lmhead_workspace_bytes(256, V) / 256;
    long rb = budget / per_row / 256 * 256;
    if (rb < 256) rb = 256;
    (void)H;
    return (int)(rb < R ? rb : R);
}

extern "C" int vlr_lmhead_ce_bwd(const void* hg, const void* w_lm, const int* tgt, const float* lse, const float* coef, void* dlogits,
                                 void* workspace, float* logits_ws, void* dhg, void* dw_lm, int dw_accumulate, int R, int V, int H,
                                 int row_block, hipStream_t st) {
    VLR_REQUIRE(hg && w_lm && tgt && lse && coef && dlogits && dhg, "vlr_lmhead_ce_bwd: null operand");
    VLR_REQUIRE(R > 0 && V % 8 == 0 && H % 8 == 0, "vlr_lmhead_ce_bwd: bad shape R=%d V=%d H=%d", R, V, H);
    if (row_block <= 0) row_block = vlr_lmhead_ce_row_block(R, V, H);
    const bf16_t* hgp = (const bf16_t*)hg;
    bf16_t* dhp = (bf16_t*)dhg;
    for (int r0 = 0, blk = 0; r0 < R; r0 += row_block, ++blk) {
        const int n = R - r0 < row_block ? R - r0 : row_block;
        // the uniform row gradient as ONE "sequence" whose d logp is *coef (no averaging): the offsets are then never read
        int rc = vlr_lmhead_logps_bwd(hgp + (size_t)r0 * H, w_lm, tgt + r0, lse + r0, tgt, 1, coef, 0, dlogits, workspace, logits_ws, n, V, H,
                                      st);
        if (rc != VLR_OK) return rc;
        rc = vlr_gemm_bf16(1, dlogits, w_lm, dhp + (size_t)r0 * H, nullptr, nullptr, n, H, V, V, H, H, 0, 0, 0, 0, st);
        if (rc != VLR_OK) return rc;
        if (dw_lm) {
            rc = vlr_gemm_bf16(2, dlogits, hgp + (size_t)r0 * H, dw_lm, nullptr, nullptr, V, H, n, V, H, H, 0, 0, (dw_accumulate || blk > 0) ? 1 : 0,
                               0, st);
            if (rc != VLR_OK) return rc;
        }
    }
    return VLR_OK;
}
