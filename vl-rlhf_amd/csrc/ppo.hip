// PPO's own arithmetic (gfx950): rewards + GAE + whitening, the clipped policy / value loss with its gradients, and the backward of the
// per-token value head.  The step restated in include/vlr.h is trl 0.8.1's; all per-token tensors are compact [R] fp32 over the response
// rows of vlr_build_rows, seq_off [n + 1] delimits the sequences.  No atomics anywhere: every reduction runs in an order fixed by the
// sizes (R, n, seq_off, H) alone, so two calls give the same bits.  exp is expf, never the fast intrinsic.
#include "../../include/vlr.h"
#include "common.h"

#define PPO_THREADS 1024

// sum of x[0..R) over the workgroup: thread t adds elements t, t + 1024, ... in that order, block_sum folds the 1024 partials
__device__ __forceinline__ float ppo_sum(const float* x, int R, float* red) {
    float s = 0.f;
    for (int i = threadIdx.x; i < R; i += PPO_THREADS) s += x[i];
    return block_sum(s, red);
}
// masked_whiten's moments over all R tokens: mean, and the biased variance around it times R / (R - 1)
__device__ __forceinline__ void ppo_moments(const float* x, int R, float* red, float& mean, float& var) {
    mean = ppo_sum(x, R, red) / (float)R;
    float s = 0.f;
    for (int i = threadIdx.x; i < R; i += PPO_THREADS) {
        const float d = x[i] - mean;
        s = fmaf(d, d, s);
    }
    var = block_sum(s, red) / (float)R * ((float)R / (float)(R - 1));
}

// ------------------------------------------------------------------------------------------------------------
// vlr_ppo_advantages.  Geometry: ONE workgroup of 1024 threads (the data is 64 x 512 tokens at most in the reference recipe: four
// [R] fp32 arrays, a few hundred kilobytes).  Phases, separated by workgroup barriers:
//   1. rewards: wave w owns sequences w, w + 16, ...; its lanes stride the sequence's tokens, write the non-score reward
//      -kl_coef * kl_t into `returns` (scratch until phase 3), fold the sequence's KL sum with xor butterflies, lane 0 adds the score
//      to the last token;
//   2. whiten_rewards: masked_whiten(shift_mean = False) over all R tokens, in place;
//   3. GAE: thread s owns sequence s (s + 1024, ...) and walks it backwards, four tokens per round of loads;
//   4. advantages <- masked_whiten(advantages); stats.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PPO_THREADS) void ppo_advantages_kernel(const float* __restrict__ old_logp, const float* __restrict__ ref_logp,
                                                                     const float* __restrict__ values, const int* __restrict__ seq_off,
                                                                     const float* __restrict__ scores, float kl_coef, int kl_penalty,
                                                                     float gamma, float lam, int whiten_rewards, float* adv, float* ret,
                                                                     float* __restrict__ kl_sums, float* __restrict__ stats, int R, int n) {
    __shared__ float red[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float nsr = 0.f;      // this lane's share of the sum of the non-score rewards
    for (int s = wave; s < n; s += PPO_THREADS / 64) {
        const int lo = max(seq_off[s], 0), hi = min(seq_off[s + 1], R);
        float ks = 0.f;
        for (int i = lo + lane; i < hi; i += 64) {
            const float d = old_logp[i] - ref_logp[i];
            const float kl = kl_penalty == 0 ? d : (kl_penalty == 1 ? fabsf(d) : 0.5f * d * d);
            const float r = -kl_coef * kl;
            ks += kl;
            nsr += r;
            ret[i] = (i == hi - 1) ? r + scores[s] : r;
        }
        ks = wave_sum(ks);
        if (lane == 0) kl_sums[s] = ks;
    }
    nsr = block_sum(nsr, red);      // (its barriers also publish phase 1's stores to the workgroup)
    if (whiten_rewards) {
        float mean, var;
        ppo_moments(ret, R, red, mean, var);
        const float rs = 1.f / sqrtf(var + 1e-8f);
        for (int i = tid; i < R; i += PPO_THREADS) ret[i] = (ret[i] - mean) * rs + mean;
    }
    __syncthreads();
    const float gl = gamma * lam;
    for (int s = tid; s < n; s += PPO_THREADS) {
        const int lo = max(seq_off[s], 0), hi = min(seq_off[s + 1], R);
        float A = 0.f, Vn = 0.f;
        int t = hi - 1;
        for (; t - 3 >= lo; t -= 4) {
            float r[4], v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                r[k] = ret[t - k];
                v[k] = values[t - k];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float delta = r[k] + gamma * Vn - v[k];
                A = delta + gl * A;
                adv[t - k] = A;
                ret[t - k] = A + v[k];
                Vn = v[k];
            }
        }
        for (; t >= lo; --t) {
            const float r = ret[t], v = values[t];
            const float delta = r + gamma * Vn - v;
            A = delta + gl * A;
            adv[t] = A;
            ret[t] = A + v;
            Vn = v;
        }
    }
    __syncthreads();
    float mean, var;
    ppo_moments(adv, R, red, mean, var);
    const float rs = 1.f / sqrtf(var + 1e-8f);
    for (int i = tid; i < R; i += PPO_THREADS) adv[i] = (adv[i] - mean) * rs;
    const float klm = ppo_sum(kl_sums, n, red) / (float)n;
    if (tid == 0) {
        stats[0] = klm;
        stats[1] = nsr / (float)R;
        stats[2] = mean;
        stats[3] = var;
    }
}

extern "C" int vlr_ppo_advantages(const float* old_logp, const float* ref_logp, const float* values, const int* seq_off,
                                  const float* scores, float kl_coef, int kl_penalty, float gamma, float lam, int whiten_rewards,
                                  float* advantages, float* returns, float* kl_sums, float* stats, int R, int n, hipStream_t st) {
    VLR_REQUIRE(old_logp && ref_logp && values && seq_off && scores && advantages && returns && kl_sums && stats,
                "vlr_ppo_advantages: null operand");
    VLR_REQUIRE(kl_penalty >= 0 && kl_penalty <= 2, "vlr_ppo_advantages: kl_penalty %d (0 kl, 1 abs, 2 mse; 'full' needs [R][V] logits)",
                kl_penalty);
    VLR_REQUIRE(R >= 2 && n >= 1 && n <= R, "vlr_ppo_advantages: bad shape R=%d n=%d (whitening needs R >= 2)", R, n);
    hipLaunchKernelGGL(ppo_advantages_kernel, dim3(1), dim3(PPO_THREADS), 0, st, old_logp, ref_logp, values, seq_off, scores, kl_coef,
                       kl_penalty, gamma, lam, whiten_rewards ? 1 : 0, advantages, returns, kl_sums, stats, R, n);
    return vlr_check_launch("vlr_ppo_advantages");
}

// ------------------------------------------------------------------------------------------------------------
// vlr_ppo_loss: forward, stats and both gradients in one launch.  Geometry: ONE workgroup of 1024 threads - the ratio-threshold test
// needs mean(ratio) over all R tokens before any gradient may be written, and one workgroup settles that with a barrier instead of a
// second launch or a host read.  Pass 1 folds the sums (thread t owns tokens t, t + 1024, ...), pass 2 recomputes each token and writes
// its gradients (or zeros).  Derivatives are torch autograd's: clamp passes the gradient on its closed interval, max halves a tie.
// ------------------------------------------------------------------------------------------------------------
struct ppo_tok {
    float ratio, pg, vf, dpg, dvf;      // pg = max(-A ratio, -A clip(ratio)), vf = max((v - ret)^2, (vclip - ret)^2), d pg / d logp, d vf / d vpred
    int pg_clipped, vf_clipped;
};
__device__ __forceinline__ ppo_tok ppo_token(float logp, float vpred, float old_logp, float old_v, float A, float ret, float lo, float hi,
                                             float crv) {
    ppo_tok o;
    o.ratio = expf(logp - old_logp);
    const float rc = fminf(fmaxf(o.ratio, lo), hi);
    const float a = -A * o.ratio, b = -A * rc;
    const float da = a, db = (o.ratio >= lo && o.ratio <= hi) ? a : 0.f;      // d ratio / d logp = ratio
    o.pg = fmaxf(a, b);
    o.dpg = a > b ? da : (b > a ? db : 0.5f * (da + db));
    o.pg_clipped = b > a;
    const float vlo = old_v - crv, vhi = old_v + crv;
    const float vc = fminf(fmaxf(vpred, vlo), vhi);
    const float e1 = vpred - ret, e2 = vc - ret;
    const float l1 = e1 * e1, l2 = e2 * e2;
    const float d1 = 2.f * e1, d2 = (vpred >= vlo && vpred <= vhi) ? 2.f * e2 : 0.f;
    o.vf = fmaxf(l1, l2);
    o.dvf = l1 > l2 ? d1 : (l2 > l1 ? d2 : 0.5f * (d1 + d2));
    o.vf_clipped = l2 > l1;
    return o;
}

__global__ __launch_bounds__(PPO_THREADS) void ppo_loss_kernel(const float* __restrict__ logp, const float* __restrict__ vpred,
                                                               const float* __restrict__ old_logp, const float* __restrict__ old_values,
                                                               const float* __restrict__ adv, const float* __restrict__ ret, int R,
                                                               float lo, float hi, float crv, float vf_coef, float ratio_threshold,
                                                               float upstream, float* __restrict__ dlogp, float* __restrict__ dvpred,
                                                               float* __restrict__ stats) {
    __shared__ float red[16];
    const int tid = threadIdx.x;
    float s_ratio = 0.f, s_pg = 0.f, s_vf = 0.f, s_akl = 0.f, s_pkl = 0.f, s_pgc = 0.f, s_vfc = 0.f, s_err = 0.f;
    for (int i = tid; i < R; i += PPO_THREADS) {
        const ppo_tok t = ppo_token(logp[i], vpred[i], old_logp[i], old_values[i], adv[i], ret[i], lo, hi, crv);
        const float d = logp[i] - old_logp[i], e = vpred[i] - ret[i];
        s_ratio += t.ratio;
        s_pg += t.pg;
        s_vf += t.vf;
        s_akl = fmaf(d, d, s_akl);
        s_pkl -= d;
        s_pgc += (float)t.pg_clipped;
        s_vfc += (float)t.vf_clipped;
        s_err = fmaf(e, e, s_err);
    }
    const float inv = 1.f / (float)R;
    const float m_ratio = block_sum(s_ratio, red) * inv;
    const float m_pg = block_sum(s_pg, red) * inv, m_vf = 0.5f * (block_sum(s_vf, red) * inv);
    const float m_akl = 0.5f * (block_sum(s_akl, red) * inv), m_pkl = block_sum(s_pkl, red) * inv;
    const float m_pgc = block_sum(s_pgc, red) * inv, m_vfc = block_sum(s_vfc, red) * inv, m_err = block_sum(s_err, red) * inv;
    const float m_adv = ppo_sum(adv, R, red) * inv;
    float m_ret, v_ret, m_vp, v_vp, m_ov, v_ov;
    ppo_moments(ret, R, red, m_ret, v_ret);
    ppo_moments(vpred, R, red, m_vp, v_vp);
    ppo_moments(old_values, R, red, m_ov, v_ov);
    const bool skip = m_ratio > ratio_threshold;      // uniform over the workgroup: block_sum hands every thread the same bits
    const float gp = skip ? 0.f : upstream * inv, gv = skip ? 0.f : upstream * inv * vf_coef * 0.5f;
    for (int i = tid; i < R; i += PPO_THREADS) {
        if (skip) {
            dlogp[i] = 0.f;
            dvpred[i] = 0.f;
        } else {
            const ppo_tok t = ppo_token(logp[i], vpred[i], old_logp[i], old_values[i], adv[i], ret[i], lo, hi, crv);
            dlogp[i] = gp * t.dpg;
            dvpred[i] = gv * t.dvf;
        }
    }
    if (tid == 0) {
        const float pg = skip ? 0.f : m_pg, vf = skip ? 0.f : m_vf;
        stats[0] = skip ? 0.f : pg + vf_coef * vf;
        stats[1] = pg;
        stats[2] = vf;
        stats[3] = m_akl;
        stats[4] = m_pkl;
        stats[5] = m_pgc;
        stats[6] = m_vfc;
        stats[7] = m_ratio;
        stats[8] = m_ret;
        stats[9] = v_ret;
        stats[10] = m_vp;
        stats[11] = v_vp;
        stats[12] = m_err;
        stats[13] = m_adv;
        stats[14] = m_ov;
        stats[15] = v_ov;
        stats[16] = skip ? 1.f : 0.f;
    }
}

extern "C" int vlr_ppo_loss(const float* logp, const float* vpred, const float* old_logp, const float* old_values, const float* advantages,
                            const float* returns, int R, double cliprange, double cliprange_value, float vf_coef, float ratio_threshold,
                            float upstream, float* dlogp, float* dvpred, float* stats, hipStream_t st) {
    VLR_REQUIRE(logp && vpred && old_logp && old_values && advantages && returns && dlogp && dvpred && stats, "vlr_ppo_loss: null operand");
    VLR_REQUIRE(R >= 2, "vlr_ppo_loss: bad shape R=%d (the variances need R >= 2)", R);
    VLR_REQUIRE(cliprange >= 0. && cliprange_value >= 0., "vlr_ppo_loss: negative clip range %g / %g", cliprange, cliprange_value);
    // torch.clamp(ratio, 1 - cr, 1 + cr) takes Python floats: the bounds are formed in double and rounded to fp32 once
    hipLaunchKernelGGL(ppo_loss_kernel, dim3(1), dim3(PPO_THREADS), 0, st, logp, vpred, old_logp, old_values, advantages, returns, R,
                       (float)(1.0 - cliprange), (float)(1.0 + cliprange), (float)cliprange_value, vf_coef, ratio_threshold, upstream, dlogp,
                       dvpred, stats);
    return vlr_check_launch("vlr_ppo_loss");
}

// ------------------------------------------------------------------------------------------------------------
// vlr_v_head_bwd: the value head v_r = dot(hg[r], w) + b on ALL R gathered rows (the forward is vlr_rm_head_fwd with rows = 0..R-1).
// Geometry: the rows are cut into `chunks` = ceil(R / rc) chunks of rc = max(8, ceil(R / 256)) rows (at most 256 chunks, a function of R
// alone).  Kernel 1, grid (ceil(H / 8 / 64), chunks) x one wave: a lane owns one 8-element column group, walks the chunk's rows in order,
// adds g_r * w onto d hg[r] in fp32 (one bf16 rounding) and accumulates its fp32 partial of d w; lane 0 of column block 0 also folds the
// chunk's sum of g.  Kernel 2 folds the partials: a workgroup of 256 threads owns 32 column groups x 8 strands, strand j adds chunks
// j, j + 8, ... in that order, the 8 strands are added in order through LDS, the old gradient joins in fp32 when accumulating and the
// result is rounded to bf16 once.  Workgroup 0 folds d b the same way (thread-strided, then block_sum).
// ------------------------------------------------------------------------------------------------------------
#define VH_MAX_CHUNKS 256
static inline int vh_rows_per_chunk(int R) {
    const int rc = (R + VH_MAX_CHUNKS - 1) / VH_MAX_CHUNKS;
    return rc < 8 ? 8 : rc;
}
static inline int vh_chunks(int R) {
    const int rc = vh_rows_per_chunk(R);
    return (R + rc - 1) / rc;
}

__global__ __launch_bounds__(64) void v_head_bwd_rows_kernel(const bf16_t* __restrict__ hg, const bf16_t* __restrict__ w,
                                                             const float* __restrict__ g, bf16_t* __restrict__ dhg,
                                                             float* __restrict__ part_w, float* __restrict__ part_b, int rc, int R, int H) {
    const int c = (blockIdx.x * 64 + threadIdx.x) * 8;
    const int r0 = blockIdx.y * rc, r1 = min(r0 + rc, R);
    if (c < H) {
        float wf[8], acc[8];
        unpack8(*(const u32x4*)(w + c), wf);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = 0.f;
        for (int r = r0; r < r1; ++r) {
            const float gr = g[r];
            const long o = (long)r * H + c;
            float xf[8], d[8];
            unpack8(*(const u32x4*)(hg + o), xf);
            unpack8(*(const u32x4*)(dhg + o), d);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                d[k] = fmaf(gr, wf[k], d[k]);
                acc[k] = fmaf(gr, xf[k], acc[k]);
            }
            *(u32x4*)(dhg + o) = pack8(d);
        }
        float* p = part_w + (long)blockIdx.y * H + c;
        *(f32x4*)p = f32x4{acc[0], acc[1], acc[2], acc[3]};
        *(f32x4*)(p + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float s = 0.f;
        for (int r = r0; r < r1; ++r) s += g[r];
        part_b[blockIdx.y] = s;
    }
}

__global__ __launch_bounds__(256) void v_head_bwd_fold_kernel(const float* __restrict__ part_w, const float* __restrict__ part_b,
                                                              bf16_t* __restrict__ dw, bf16_t* __restrict__ db, int accumulate, int chunks,
                                                              int H) {
    __shared__ float strand[8][32][8];
    __shared__ float red[16];
    const int cg = threadIdx.x & 31, j = threadIdx.x >> 5;
    const int c = (blockIdx.x * 32 + cg) * 8;
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
    if (c < H) {
        for (int ch = j; ch < chunks; ch += 8) {
            const float* p = part_w + (long)ch * H + c;
            const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                acc[k] += a[k];
                acc[k + 4] += b[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) strand[j][cg][k] = acc[k];
    __syncthreads();
    if (j == 0 && c < H) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float s = strand[0][cg][k];
            for (int q = 1; q < 8; ++q) s += strand[q][cg][k];
            acc[k] = s;
        }
        if (accumulate) {
            float old[8];
            unpack8(*(const u32x4*)(dw + c), old);
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] += old[k];
        }
        *(u32x4*)(dw + c) = pack8(acc);
    }
    if (blockIdx.x == 0) {
        float s = 0.f;
        for (int ch = threadIdx.x; ch < chunks; ch += 256) s += part_b[ch];
        s = block_sum(s, red);
        if (threadIdx.x == 0) {
            if (accumulate) s += bf16_to_f32(db[0]);
            db[0] = f32_to_bf16(s);
        }
    }
}

extern "C" long vlr_v_head_bwd_workspace_bytes(int R, int H) {
    if (R <= 0 || H <= 0) return 0;
    return (long)vh_chunks(R) * ((long)H + 1) * 4;
}

extern "C" int vlr_v_head_bwd(const void* hg, const void* w, const float* g, void* dhg_inout, void* dw, void* db, int accumulate,
                              void* workspace, int R, int H, hipStream_t st) {
    VLR_REQUIRE(hg && w && g && dhg_inout && dw && db && workspace, "vlr_v_head_bwd: null operand");
    VLR_REQUIRE(R > 0 && H >= 8 && H % 8 == 0, "vlr_v_head_bwd: bad shape R=%d H=%d", R, H);
    const int rc = vh_rows_per_chunk(R), chunks = vh_chunks(R), groups = H / 8;
    float* part_w = (float*)workspace;
    float* part_b = part_w + (long)chunks * H;
    hipLaunchKernelGGL(v_head_bwd_rows_kernel, dim3((groups + 63) / 64, chunks), dim3(64), 0, st, (const bf16_t*)hg, (const bf16_t*)w, g,
                       (bf16_t*)dhg_inout, part_w, part_b, rc, R, H);
    hipLaunchKernelGGL(v_head_bwd_fold_kernel, dim3((groups + 31) / 32), dim3(256), 0, st, (const float*)part_w, (const float*)part_b,
                       (bf16_t*)dw, (bf16_t*)db, accumulate ? 1 : 0, chunks, H);
    return vlr_check_launch("vlr_v_head_bwd");
}
