// KTO's own arithmetic (gfx950): the loss of Kahneman-Tversky Optimization on unpaired rows with its statistics and its gradient in one
// launch (include/vlr.h "KTO").  The inputs are summed completion log-probs: n main rows with a label, m KL rows.
// No atomics anywhere: every reduction runs in an order fixed by n and m alone, so two calls give the same bits.  exp is expf, never the
// fast intrinsic.
#include "../../include/vlr.h"
#include "common.h"

#include <math.h>

#define KTO_THREADS 1024
#define KTO_MAX_ROWS (1 << 20)

// ------------------------------------------------------------------------------------------------------------
// vlr_kto_loss.  Geometry: ONE workgroup of 1024 threads (a batch is a handful of rows); the lanes stride the rows.  First the KL
// baseline: the mean of pi_kl - ref_kl over the m KL rows, clamped at 0 - every thread ends with the same bits of it, and nothing
// differentiates it.  Then one pass over the main rows.  With z = beta (r - kl) for a desirable row and beta (kl - r) for an undesirable
// one, q = 1 - sigmoid(z) is formed as 1 / (1 + expf(z)): it keeps its relative accuracy where sigmoid(z) rounds to 1, and a saturated
// z gives q = 0 (expf = inf) or q = 1 (expf = 0) and q (1 - q) = 0 exactly, never NaN.  Each sum is per-lane partials, six xor butterflies,
// then the 16 waves in order.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KTO_THREADS) void kto_loss_kernel(const float* __restrict__ pi, const float* __restrict__ ref,
                                                               const unsigned char* __restrict__ label, int n,
                                                               const float* __restrict__ pi_kl, const float* __restrict__ ref_kl, int m,
                                                               float beta, float c_d, float c_u, float w_d, float w_u,
                                                               float* __restrict__ losses, float* __restrict__ rewards,
                                                               float* __restrict__ dpi, float* __restrict__ stats) {
    __shared__ float red[16];
    const int tid = threadIdx.x;
    float s_kl = 0.f;
    for (int j = tid; j < m; j += KTO_THREADS) s_kl += pi_kl[j] - ref_kl[j];
    const float kl = fmaxf(block_sum(s_kl, red) / (float)m, 0.f);
    float s_l = 0.f, s_rd = 0.f, s_ru = 0.f, s_pd = 0.f, s_pu = 0.f, s_nd = 0.f;
    for (int i = tid; i < n; i += KTO_THREADS) {
        const float p = pi[i];
        const float r = p - ref[i];
        const bool d = label[i] != 0;
        const float z = d ? beta * (r - kl) : beta * (kl - r);
        const float q = 1.f / (1.f + expf(z));
        const float l = (d ? w_d : w_u) * q;
        const float rw = beta * r;
        losses[i] = l;
        rewards[i] = rw;
        dpi[i] = (d ? -c_d : c_u) * (q * (1.f - q));
        s_l += l;
        s_rd += d ? rw : 0.f;
        s_ru += d ? 0.f : rw;
        s_pd += d ? p : 0.f;
        s_pu += d ? 0.f : p;
        s_nd += d ? 1.f : 0.f;
    }
    const float t_l = block_sum(s_l, red), t_rd = block_sum(s_rd, red), t_ru = block_sum(s_ru, red);
    const float t_pd = block_sum(s_pd, red), t_pu = block_sum(s_pu, red), t_nd = block_sum(s_nd, red);
    if (tid == 0) {
        stats[0] = t_l / (float)n;
        stats[1] = kl;
        stats[2] = t_rd;
        stats[3] = t_ru;
        stats[4] = t_pd;
        stats[5] = t_pu;
        stats[6] = t_nd;
        stats[7] = (float)n - t_nd;
    }
}

extern "C" int vlr_kto_loss(const float* pi, const float* ref, const unsigned char* label, int n, const float* pi_kl, const float* ref_kl,
                            int m, float beta, float w_desirable, float w_undesirable, float upstream, float* losses, float* rewards,
                            float* dpi, float* stats, hipStream_t st) {
    VLR_REQUIRE(pi && ref && label && pi_kl && ref_kl && losses && rewards && dpi && stats, "vlr_kto_loss: null operand");
    VLR_REQUIRE(n >= 1 && n <= KTO_MAX_ROWS && m >= 1 && m <= KTO_MAX_ROWS, "vlr_kto_loss: bad shape n=%d m=%d (1 .. 2^20 rows each)", n, m);
    VLR_REQUIRE(isfinite(beta) && isfinite(w_desirable) && isfinite(w_undesirable) && isfinite(upstream),
                "vlr_kto_loss: beta %g, weights %g / %g or upstream %g is not finite", (double)beta, (double)w_desirable,
                (double)w_undesirable, (double)upstream);
    // the gradient's weight, in this order: ((w beta) / n) upstream
    const float c_d = w_desirable * beta / (float)n * upstream, c_u = w_undesirable * beta / (float)n * upstream;
    hipLaunchKernelGGL(kto_loss_kernel, dim3(1), dim3(KTO_THREADS), 0, st, pi, ref, label, n, pi_kl, ref_kl, m, beta, c_d, c_u, w_desirable,
                       w_undesirable, losses, rewards, dpi, stats);
    return vlr_check_launch("vlr_kto_loss");
}
