// Reward-model head (gfx950): rm_head = nn.Linear(hidden, 1) read at ONE row per sequence (reference base/model.py VLRewardModel:
// rm_head(hidden_states[-1][:, -1, :])).  n is the batch size, so both kernels are tiny; what they owe the trainer is a fixed reduction
// order (a row's reward has the same bits alone or inside a batch, and from call to call) and gradients summed in fp32 in the order of
// the rows, rounded to bf16 once.  No atomics.
#include "../../include/vlr.h"
#include "common.h"

// ------------------------------------------------------------------------------------------------------------
// rewards[i] = dot(hidden[rows[i]], w) + b: one workgroup per reward row.  Thread t owns the 8-element chunks t, t + 256, ... and adds
// them in that order; the 256 partials are folded by block_sum (xor butterflies inside a wave, then the 4 waves in order).  Nothing in
// that order depends on n or on the block index.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rm_head_fwd_kernel(const bf16_t* __restrict__ hidden, long ldh, const int* __restrict__ rows,
                                                          const bf16_t* __restrict__ w, const bf16_t* __restrict__ b,
                                                          float* __restrict__ rewards, int H) {
    __shared__ float red[16];
    const bf16_t* x = hidden + (long)rows[blockIdx.x] * ldh;
    float s = 0.f;
    for (int c = threadIdx.x * 8; c < H; c += 256 * 8) {
        const u32x4 xv = *(const u32x4*)(x + c);
        const u32x4 wv = *(const u32x4*)(w + c);
        float xf[8], wf[8];
        unpack8(xv, xf);
        unpack8(wv, wf);
#pragma unroll
        for (int k = 0; k < 8; ++k) s = fmaf(xf[k], wf[k], s);
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) rewards[blockIdx.x] = s + bf16_to_f32(b[0]);
}

extern "C" int vlr_rm_head_fwd(const void* hidden, int ldh, const int* rows, const void* w, const void* b, float* rewards, int n, int H,
                               hipStream_t st) {
    VLR_REQUIRE(hidden && rows && w && b && rewards, "vlr_rm_head_fwd: null operand");
    VLR_REQUIRE(n > 0 && H >= 8 && H % 8 == 0 && ldh >= H && ldh % 8 == 0, "vlr_rm_head_fwd: bad shape n=%d H=%d ldh=%d", n, H, ldh);
    hipLaunchKernelGGL(rm_head_fwd_kernel, dim3(n), dim3(256), 0, st, (const bf16_t*)hidden, (long)ldh, rows, (const bf16_t*)w,
                       (const bf16_t*)b, rewards, H);
    return vlr_check_launch("vlr_rm_head_fwd");
}

// ------------------------------------------------------------------------------------------------------------
// Backward.  One thread per 8-element chunk of H walks the n reward rows in order: it writes its chunk of
// d hidden[rows[i]] = bf16(g_i * w) and adds g_i * hidden[rows[i]] to its fp32 chunk of d w; the chunk is rounded to bf16 once (after
// the old gradient was added in fp32, when accumulating).  Thread 0 of block 0 folds d b = sum_i g_i the same way.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rm_head_bwd_kernel(const bf16_t* __restrict__ hidden, long ldh, const int* __restrict__ rows,
                                                          const bf16_t* __restrict__ w, const float* __restrict__ g,
                                                          bf16_t* __restrict__ dhidden, long ldd, bf16_t* __restrict__ dw,
                                                          bf16_t* __restrict__ db, int accumulate, int n, int H) {
    const int c = (blockIdx.x * 256 + threadIdx.x) * 8;
    if (c < H) {
        float wf[8], acc[8];
        unpack8(*(const u32x4*)(w + c), wf);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = 0.f;
        for (int i = 0; i < n; ++i) {
            const long r = rows[i];
            const float gi = g[i];
            float xf[8], d[8];
            unpack8(*(const u32x4*)(hidden + r * ldh + c), xf);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                d[k] = gi * wf[k];
                acc[k] = fmaf(gi, xf[k], acc[k]);
            }
            *(u32x4*)(dhidden + r * ldd + c) = pack8(d);
        }
        if (accumulate) {
            float old[8];
            unpack8(*(const u32x4*)(dw + c), old);
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] += old[k];
        }
        *(u32x4*)(dw + c) = pack8(acc);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < n; ++i) s += g[i];
        if (accumulate) s += bf16_to_f32(db[0]);
        db[0] = f32_to_bf16(s);
    }
}

extern "C" int vlr_rm_head_bwd(const void* hidden, int ldh, const int* rows, const void* w, const float* d_rewards, void* dhidden, int ldd,
                               void* dw, void* db, int accumulate, int n, int H, hipStream_t st) {
    VLR_REQUIRE(hidden && rows && w && d_rewards && dhidden && dw && db, "vlr_rm_head_bwd: null operand");
    VLR_REQUIRE(n > 0 && H >= 8 && H % 8 == 0 && ldh >= H && ldh % 8 == 0 && ldd >= H && ldd % 8 == 0,
                "vlr_rm_head_bwd: bad shape n=%d H=%d ldh=%d ldd=%d", n, H, ldh, ldd);
    const int chunks = H / 8;
    hipLaunchKernelGGL(rm_head_bwd_kernel, dim3((chunks + 255) / 256), dim3(256), 0, st, (const bf16_t*)hidden, (long)ldh, rows,
                       (const bf16_t*)w, d_rewards, (bf16_t*)dhidden, (long)ldd, (bf16_t*)dw, (bf16_t*)db, accumulate ? 1 : 0, n, H);
    return vlr_check_launch("vlr_rm_head_bwd");
}
