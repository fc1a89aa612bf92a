// GRPO's own arithmetic (gfx950): the group-standardised advantages and the clipped per-token loss with its gradient (include/vlr.h
// "GRPO").  The per-token tensors are compact [R] fp32 over the response rows of vlr_build_rows, seq_off [n + 1] delimits the sequences.
// No atomics anywhere: every reduction runs in an order fixed by the sizes (P, G, R, n, seq_off) alone, so two calls give the same bits.
// exp is expf, never the fast intrinsic.
#include "../../include/vlr.h"
#include "common.h"

#define GRPO_THREADS 1024
#define GRPO_WAVES (GRPO_THREADS / 64)

// ------------------------------------------------------------------------------------------------------------
// vlr_grpo_advantages.  Geometry: ONE workgroup of 1024 threads (P x G scores: a few hundred floats).  Wave w owns the groups w, w + 16,
// ...; its lanes stride the group's G scores.  The moments are taken of d_j = s_j - s_0, the scores shifted by the group's first one: the
// mean is s_0 + sum(d) / G, the deviation e_j = d_j - sum(d) / G, and a group of equal scores has d = 0, so e = 0 and std = 0 exactly,
// whatever sum(s) / G would have rounded to.  Each sum is lane-strided partials folded by six xor butterflies (every lane ends with the
// same bits).  The three statistics are per-wave sums over the wave's groups in order, folded over the 16 waves in order.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GRPO_THREADS) void grpo_advantages_kernel(const float* __restrict__ scores, int P, int G, int scale,
                                                                       float* __restrict__ adv, float* __restrict__ stats) {
    __shared__ float red[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float s_mean = 0.f, s_std = 0.f, s_zero = 0.f;      // wave-uniform: sums over this wave's groups
    for (int p = wave; p < P; p += GRPO_WAVES) {
        const float* s = scores + (long)p * G;
        float* a = adv + (long)p * G;
        const float c = s[0];
        float sd = 0.f;
        for (int j = lane; j < G; j += 64) sd += s[j] - c;
        const float m = wave_sum(sd) / (float)G;
        float sq = 0.f;
        for (int j = lane; j < G; j += 64) {
            const float e = (s[j] - c) - m;
            sq = fmaf(e, e, sq);
        }
        const float sdev = sqrtf(wave_sum(sq) / (float)(G - 1));
        const float den = sdev + 1e-4f;
        for (int j = lane; j < G; j += 64) {
            const float e = (s[j] - c) - m;
            a[j] = scale ? e / den : e;
        }
        s_mean += c + m;
        s_std += sdev;
        s_zero += sdev == 0.f ? 1.f : 0.f;
    }
    const float t_mean = block_sum(lane == 0 ? s_mean : 0.f, red);
    const float t_std = block_sum(lane == 0 ? s_std : 0.f, red);
    const float t_zero = block_sum(lane == 0 ? s_zero : 0.f, red);
    if (tid == 0) {
        stats[0] = t_mean / (float)P;
        stats[1] = t_std / (float)P;
        stats[2] = t_zero / (float)P;
        stats[3] = 0.f;
    }
}

extern "C" int vlr_grpo_advantages(const float* scores, int P, int G, int scale_rewards, float* advantages, float* stats, hipStream_t st) {
    VLR_REQUIRE(scores && advantages && stats, "vlr_grpo_advantages: null operand");
    VLR_REQUIRE(P >= 1 && G >= 2 && (long)P * G <= 0x7fffffffL, "vlr_grpo_advantages: bad shape P=%d G=%d (the unbiased std needs G >= 2)", P, G);
    hipLaunchKernelGGL(grpo_advantages_kernel, dim3(1), dim3(GRPO_THREADS), 0, st, scores, P, G, scale_rewards ? 1 : 0, advantages, stats);
    return vlr_check_launch("vlr_grpo_advantages");
}

// ------------------------------------------------------------------------------------------------------------
// vlr_grpo_loss: forward, stats and the gradient in one launch and one pass.  Geometry: ONE workgroup of 1024 threads; wave w owns the
// sequences w, w + 16, ... and its lanes stride the sequence's tokens, so a token knows its sequence (its advantage, its length) without
// a search in seq_off.  Every weight a gradient needs is known before the sums are: 1 / (n len_s), 1 / R or 1 / (n max_completion_length).
// Per sequence the token losses are folded by xor butterflies (loss_type 0 divides by len_s there); the per-lane token sums and the
// per-wave sequence sums are folded over the workgroup at the end.  Derivatives are torch autograd's: clamp passes the gradient on its
// closed interval, min halves a tie.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GRPO_THREADS) void grpo_loss_kernel(const float* __restrict__ logp, const float* __restrict__ old_logp,
                                                                 const float* __restrict__ ref_logp, const float* __restrict__ adv_seq,
                                                                 const int* __restrict__ seq_off, int R, int n, float lo, float hi, float beta,
                                                                 int loss_type, float inv_norm, float upstream, float* __restrict__ dlogp,
                                                                 float* __restrict__ stats) {
    __shared__ float red[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float s_l = 0.f, s_kl = 0.f, s_lo = 0.f, s_hi = 0.f, s_ratio = 0.f;      // this lane's token sums
    float s_seq = 0.f;                                                       // wave-uniform: sum of the wave's sequence means (loss_type 0)
    for (int s = wave; s < n; s += GRPO_WAVES) {
        const int b = max(seq_off[s], 0), e = min(seq_off[s + 1], R);
        if (e <= b) continue;      // (uniform over the wave)
        const float A = adv_seq[s];
        const float inv_len = 1.f / (float)(e - b);
        const float g = upstream * (loss_type == 0 ? inv_norm * inv_len : inv_norm);
        float sl = 0.f;
        for (int i = b + lane; i < e; i += 64) {
            const float lp = logp[i];
            const float r = expf(lp - (old_logp ? old_logp[i] : lp));
            const float rc = fminf(fmaxf(r, lo), hi);
            const float u = r * A, c = rc * A;
            const float du = u, dc = (r >= lo && r <= hi) ? u : 0.f;      // d ratio / d logp = ratio
            float l = -fminf(u, c);
            float dl = -(u < c ? du : (c < u ? dc : 0.5f * (du + dc)));
            if (beta != 0.f) {
                const float d = ref_logp[i] - lp;
                const float ed = expf(d);
                const float k = ed - d - 1.f;
                l = fmaf(beta, k, l);
                dl = fmaf(beta, 1.f - ed, dl);
                s_kl += k;
            }
            dlogp[i] = g * dl;
            sl += l;
            s_lo += (r < lo && A < 0.f) ? 1.f : 0.f;
            s_hi += (r > hi && A > 0.f) ? 1.f : 0.f;
            s_ratio += r;
        }
        s_l += sl;
        if (loss_type == 0) s_seq += wave_sum(sl) * inv_len;
    }
    const float invR = 1.f / (float)R;
    const float t_l = block_sum(s_l, red), t_seq = block_sum(lane == 0 ? s_seq : 0.f, red);
    const float m_kl = block_sum(s_kl, red) * invR, m_lo = block_sum(s_lo, red) * invR, m_hi = block_sum(s_hi, red) * invR;
    const float m_ratio = block_sum(s_ratio, red) * invR;
    if (tid == 0) {
        stats[0] = (loss_type == 0 ? t_seq : t_l) * inv_norm;
        stats[1] = m_kl;
        stats[2] = m_lo;
        stats[3] = m_hi;
        stats[4] = m_lo + m_hi;
        stats[5] = m_ratio;
        stats[6] = (float)R / (float)n;
        stats[7] = 0.f;
    }
}

extern "C" int vlr_grpo_loss(const float* logp, const float* old_logp, const float* ref_logp, const float* adv_seq, const int* seq_off, int R,
                             int n, double eps_low, double eps_high, float beta, int loss_type, int max_completion_length, float upstream,
                             float* dlogp, float* stats, hipStream_t st) {
    VLR_REQUIRE(logp && adv_seq && seq_off && dlogp && stats, "vlr_grpo_loss: null operand");
    VLR_REQUIRE(ref_logp || beta == 0.f, "vlr_grpo_loss: null ref_logp with beta %g (the KL term needs the reference)", (double)beta);
    VLR_REQUIRE(R >= 1 && n >= 1 && n <= R, "vlr_grpo_loss: bad shape R=%d n=%d", R, n);
    VLR_REQUIRE(eps_low >= 0. && eps_high >= 0., "vlr_grpo_loss: negative clip range %g / %g", eps_low, eps_high);
    VLR_REQUIRE(loss_type >= 0 && loss_type <= 2, "vlr_grpo_loss: loss_type %d (0 grpo, 1 bnpo, 2 dr_grpo)", loss_type);
    VLR_REQUIRE(loss_type != 2 || max_completion_length >= 1, "vlr_grpo_loss: max_completion_length %d with loss_type 2 (dr_grpo)",
                max_completion_length);
    // torch.clamp(ratio, 1 - eps_low, 1 + eps_high) takes Python floats: the bounds are formed in double and rounded to fp32 once
    const float inv_norm = loss_type == 0 ? 1.f / (float)n : (loss_type == 1 ? 1.f / (float)R : 1.f / ((float)n * (float)max_completion_length));
    hipLaunchKernelGGL(grpo_loss_kernel, dim3(1), dim3(GRPO_THREADS), 0, st, logp, old_logp, ref_logp, adv_seq, seq_off, R, n,
                       (float)(1.0 - eps_low), (float)(1.0 + eps_high), beta, loss_type, inv_norm, upstream, dlogp, stats);
    return vlr_check_launch("vlr_grpo_loss");
}

// ------------------------------------------------------------------------------------------------------------
// vlr_grpo_loss_ent: grpo_loss_kernel's pass with the per-token entropy H_t, the keep mask and the bonus (include/vlr.h).  The statements
// that form a token's loss and gradient are grpo_loss_kernel's; keep_t (1 or 0) multiplies them afterwards and the bonus is subtracted
// last, so keep = NULL and entropy_coef = 0 leave every bit (x 1 and - 0 * H).  The KL, clip and ratio statistics count every token.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GRPO_THREADS) void grpo_loss_ent_kernel(const float* __restrict__ logp, const float* __restrict__ old_logp,
                                                                     const float* __restrict__ ref_logp, const float* __restrict__ adv_seq,
                                                                     const int* __restrict__ seq_off, int R, int n, float lo, float hi,
                                                                     float beta, int loss_type, float inv_norm, float upstream,
                                                                     const float* __restrict__ entropy, const unsigned char* __restrict__ keep,
                                                                     float coef, float* __restrict__ dlogp, float* __restrict__ dent,
                                                                     float* __restrict__ stats) {
    __shared__ float red[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float s_l = 0.f, s_kl = 0.f, s_lo = 0.f, s_hi = 0.f, s_ratio = 0.f, s_h = 0.f, s_keep = 0.f;      // this lane's token sums
    float s_seq = 0.f;                                                       // wave-uniform: sum of the wave's sequence means (loss_type 0)
    for (int s = wave; s < n; s += GRPO_WAVES) {
        const int b = max(seq_off[s], 0), e = min(seq_off[s + 1], R);
        if (e <= b) continue;      // (uniform over the wave)
        const float A = adv_seq[s];
        const float inv_len = 1.f / (float)(e - b);
        const float g = upstream * (loss_type == 0 ? inv_norm * inv_len : inv_norm);
        float sl = 0.f;
        for (int i = b + lane; i < e; i += 64) {
            const float lp = logp[i];
            const float r = expf(lp - (old_logp ? old_logp[i] : lp));
            const float rc = fminf(fmaxf(r, lo), hi);
            const float u = r * A, c = rc * A;
            const float du = u, dc = (r >= lo && r <= hi) ? u : 0.f;      // d ratio / d logp = ratio
            float l = -fminf(u, c);
            float dl = -(u < c ? du : (c < u ? dc : 0.5f * (du + dc)));
            if (beta != 0.f) {
                const float d = ref_logp[i] - lp;
                const float ed = expf(d);
                const float k = ed - d - 1.f;
                l = fmaf(beta, k, l);
                dl = fmaf(beta, 1.f - ed, dl);
                s_kl += k;
            }
            const bool kept = !keep || keep[i] != 0;
            const float h = entropy ? entropy[i] : 0.f;
            dlogp[i] = kept ? g * dl : 0.f;
            if (dent) dent[i] = -(coef * g);
            if (!kept) l = 0.f;
            if (coef != 0.f) l -= coef * h;
            sl += l;
            s_lo += (r < lo && A < 0.f) ? 1.f : 0.f;
            s_hi += (r > hi && A > 0.f) ? 1.f : 0.f;
            s_ratio += r;
            s_h += h;
            s_keep += kept ? 1.f : 0.f;
        }
        s_l += sl;
        if (loss_type == 0) s_seq += wave_sum(sl) * inv_len;
    }
    const float invR = 1.f / (float)R;
    const float t_l = block_sum(s_l, red), t_seq = block_sum(lane == 0 ? s_seq : 0.f, red);
    const float m_kl = block_sum(s_kl, red) * invR, m_lo = block_sum(s_lo, red) * invR, m_hi = block_sum(s_hi, red) * invR;
    const float m_ratio = block_sum(s_ratio, red) * invR;
    const float m_h = block_sum(s_h, red) * invR, m_keep = block_sum(s_keep, red) * invR;
    if (tid == 0) {
        stats[0] = (loss_type == 0 ? t_seq : t_l) * inv_norm;
        stats[1] = m_kl;
        stats[2] = m_lo;
        stats[3] = m_hi;
        stats[4] = m_lo + m_hi;
        stats[5] = m_ratio;
        stats[6] = (float)R / (float)n;
        stats[7] = 0.f;
        stats[8] = m_h;
        stats[9] = m_keep;
    }
}

extern "C" int vlr_grpo_loss_ent(const float* logp, const float* old_logp, const float* ref_logp, const float* adv_seq, const int* seq_off,
                                 int R, int n, double eps_low, double eps_high, float beta, int loss_type, int max_completion_length,
                                 float upstream, const float* entropy, const unsigned char* keep, float entropy_coef, float* dlogp,
                                 float* dent, float* stats, hipStream_t st) {
    VLR_REQUIRE(logp && adv_seq && seq_off && dlogp && stats, "vlr_grpo_loss_ent: null operand");
    VLR_REQUIRE(ref_logp || beta == 0.f, "vlr_grpo_loss_ent: null ref_logp with beta %g (the KL term needs the reference)", (double)beta);
    VLR_REQUIRE((entropy && dent) || entropy_coef == 0.f, "vlr_grpo_loss_ent: null entropy / dent with entropy_coef %g", (double)entropy_coef);
    VLR_REQUIRE(R >= 1 && n >= 1 && n <= R, "vlr_grpo_loss_ent: bad shape R=%d n=%d", R, n);
    VLR_REQUIRE(eps_low >= 0. && eps_high >= 0., "vlr_grpo_loss_ent: negative clip range %g / %g", eps_low, eps_high);
    VLR_REQUIRE(loss_type >= 0 && loss_type <= 2, "vlr_grpo_loss_ent: loss_type %d (0 grpo, 1 bnpo, 2 dr_grpo)", loss_type);
    VLR_REQUIRE(loss_type != 2 || max_completion_length >= 1, "vlr_grpo_loss_ent: max_completion_length %d with loss_type 2 (dr_grpo)",
                max_completion_length);
    const float inv_norm = loss_type == 0 ? 1.f / (float)n : (loss_type == 1 ? 1.f / (float)R : 1.f / ((float)n * (float)max_completion_length));
    hipLaunchKernelGGL(grpo_loss_ent_kernel, dim3(1), dim3(GRPO_THREADS), 0, st, logp, old_logp, ref_logp, adv_seq, seq_off, R, n,
                       (float)(1.0 - eps_low), (float)(1.0 + eps_high), beta, loss_type, inv_norm, upstream, entropy, keep, entropy_coef, dlogp,
                       dent, stats);
    return vlr_check_launch("vlr_grpo_loss_ent");
}
