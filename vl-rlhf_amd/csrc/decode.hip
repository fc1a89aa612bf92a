// KV-cache decoding: one new token per sequence against a per-layer K/V cache (transformers LlamaAttention with a DynamicCache
// during `generate`).  Every kernel here is bound by HBM bandwidth, not by the matrix pipe:
//
//   gemv_kernel          Y [M][N] = X [M][K] . W [N][K]^T for M <= 16 - the weight matrix is streamed ONCE.  One MFMA
//                        (v_mfma_f32_16x16x32_bf16) per 16 x 16 x 32 block with M padded to 16: a lane's W operand is one 16-byte
//                        load, the X operand one more that four n tiles share, so the whole inner loop is 16-byte loads and four
//                        MFMAs per k step.  VALU dot products would need M x 8 FMAs plus the bf16 unpacking per W load - at
//                        M = 16 that is as long as the load itself; the padded MFMA costs nothing the loads do not already hide.
//                        A workgroup (4 waves) owns 64 output columns and one K slice; its waves take 128-k chunks in turn and
//                        meet in LDS in a fixed order.  K slices (split-K, enough workgroups to cover the chip at N = 4096) write
//                        fp32 partials; gemv_epilogue_kernel sums them in slice order and applies the epilogue: no atomics, the
//                        result is bit-reproducible.
//   gemv_wide_kernel     gemv_kernel for 17 .. 64 rows in ONE pass over W (batches of 32 - 64 sampled sequences): gemv_tile<MT> feeds a lane's
//                        W fragments to MT = ceil(M / 16) row tiles; grid, chunk order, folds and partial layout are gemv_kernel's, so the
//                        result is bit for bit that of gemv_kernel on rows [0, 16), [16, 32), ...  (gemv_wide_lora_kernel: with the adapter)
//   gemv_w4_kernel       the same product with W read PACKED (GPTQ int4, gptq.h): a quarter of the weight bytes.  One int32 of qweight
//                        is 8 consecutive k of one column - exactly one lane's B fragment of the MFMA - so a lane loads 16 bytes (4
//                        columns x 8 k), unpacks them to bf16 in registers by the rule of gptq.h and feeds four MFMAs.  Same partials,
//                        same epilogue kernel, same fixed summation order.  gemv_w4_kernel<PER_STEP, MT>, MT = 2 .. 4: the wide form -
//                        a fragment is unpacked once and feeds MT row tiles (17 .. 64 rows); bit for bit the MT = 1 kernel on 16-row groups
//   gemv_lora_kernel /   the two products with a live LoRA adapter: one more K slice whose workgroups write u B^T, u = bf16(scale * x A^T)
//   gemv_w4_lora_kernel  (see "live LoRA adapters" below) - the adapter term is summed last, in front of the epilogue
//   kv_cache_write_kernel  post-RoPE K / V column blocks of the fused qkv rows -> cache columns slot0 .. slot0 + S - 1 (exact copy)
//   attn_decode_kernel   flash-decoding: a workgroup owns (sequence, kv head, key chunk) and all heads / kv_heads query heads of the
//                        group, so a grouped K/V chunk is read once; partials (max, sum, fp32 accumulator) go to a workspace and
//                        attn_decode_combine_kernel folds them in chunk order.
//   attn_shared_prompt_kernel  the same for the `fanout` samples of one prompt (num_return_sequences): a workgroup owns (prompt, kv head,
//                        prompt key chunk) and ALL fanout * heads / kv_heads query rows of that prompt, so a prompt K/V chunk is read
//                        from HBM once per step and not once per sample.  Both products run on v_mfma_f32_16x16x32_bf16 (see the
//                        kernel); the samples' own tails go through attn_decode_kernel and attn_shared_combine_kernel folds prompt
//                        chunks, then tail chunks, in order.
#include "../../include/vlr.h"
#include "common.h"
#include "gptq.h"

constexpr int GV_COLS = 64;          // output columns per workgroup (4 MFMA n tiles of 16)
constexpr int GV_CHUNK = 128;        // k per chunk: 4 MFMA k steps of 32, all loads issued before the MFMAs
constexpr int GV_TARGET_WGS = 1024;  // split K until about this many workgroups are in flight (256 CUs)

__device__ __forceinline__ bf16x8 load8(const bf16_t* p) { return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(p)); }

// one workgroup's (64 columns, K slice `split`) share of the product for MT row tiles of 16 (M <= 16 MT); red: the workgroup's LDS.
// A lane's four W fragments of a k step are loaded once and feed MT x 4 MFMAs: only the X fragments and the accumulators grow with
// MT.  Row m = 16 mt + r sees the chunks, the k steps and the four-wave fold of the MT = 1 form in the same order, so its sums do not
// depend on MT.  The fold runs one row tile at a time through the same 16 KB of LDS.
template <int MT>
__device__ __forceinline__ void gemv_tile(const bf16_t* __restrict__ X, int ldx, const bf16_t* __restrict__ W, float* __restrict__ part,
                                          int M, int N, int K, int cps, int n0, int split, float (*red)[16][GV_COLS]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int nchunks = (K + GV_CHUNK - 1) / GV_CHUNK;
    const int c0 = split * cps, c1 = min(nchunks, c0 + cps);
    bool mok[MT];
    const bf16_t* xrow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        mok[mt] = 16 * mt + r < M;
        xrow[mt] = X + (size_t)(mok[mt] ? 16 * mt + r : 0) * ldx;
    }
    const bf16_t* wrow[4];
    bool nok[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int n = n0 + t * 16 + r;
        nok[t] = n < N;
        wrow[t] = W + (size_t)(nok[t] ? n : 0) * K;
    }
    f32x4 acc[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bf16x8 zero = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
    // lane (r, g) holds A[m = 16 mt + r][k = 8 g + j] (X) and B[k = 8 g + j][n = r] (a row of W) of every 32-k step
    for (int c = c0 + wv; c < c1; c += 4) {
        bf16x8 a[4][MT], b[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = c * GV_CHUNK + u * 32 + g * 8;
            const bool kok = k < K;                        // K % 8 == 0: a lane's 8 k are all in or all out
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) a[u][mt] = (mok[mt] && kok) ? load8(xrow[mt] + k) : zero;
#pragma unroll
            for (int t = 0; t < 4; ++t) b[u][t] = (nok[t] && kok) ? load8(wrow[t] + k) : zero;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u][mt], b[u][t], acc[mt][t], 0, 0, 0);
    }
    // D map: lane holds D[m = 16 mt + 4 g + i][n = r] of each n tile
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        if (mt) __syncthreads();                           // the previous row tile has been folded
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) red[wv][4 * g + i][t * 16 + r] = acc[mt][t][i];
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = threadIdx.x + 256 * e, ml = idx / GV_COLS, m = 16 * mt + ml, n = idx % GV_COLS;
            if (m < M && n0 + n < N)
                part[((size_t)split * M + m) * N + n0 + n] = ((red[0][ml][n] + red[1][ml][n]) + red[2][ml][n]) + red[3][ml][n];
        }
    }
}

__global__ __launch_bounds__(256) void gemv_kernel(const bf16_t* __restrict__ X, int ldx, const bf16_t* __restrict__ W,
                                                   float* __restrict__ part, int M, int N, int K, int cps) {
    __shared__ float red[4][16][GV_COLS];
    gemv_tile<1>(X, ldx, W, part, M, N, K, cps, blockIdx.x * GV_COLS, blockIdx.y, red);
}

// the wide form: 17 .. 64 rows (MT = 2 .. 4 row tiles) in ONE pass over W; same grid, chunk assignment and partial layout [slice][M][N]
template <int MT>
__global__ __launch_bounds__(256) void gemv_wide_kernel(const bf16_t* __restrict__ X, int ldx, const bf16_t* __restrict__ W,
                                                        float* __restrict__ part, int M, int N, int K, int cps) {
    __shared__ float red[4][16][GV_COLS];
    gemv_tile<MT>(X, ldx, W, part, M, N, K, cps, blockIdx.x * GV_COLS, blockIdx.y, red);
}

// ---- live LoRA adapters (peft lora.Linear, un-merged): y = x W^T + u B^T with u = bf16(scale * x A^T), for `targets` sub-targets
// fused along N (q|k|v: 3, gate|up: 2, o / down: 1).  A [targets * r][K], B [N][r] in the fused row order; row n of target t(n) multiplies
// columns t(n) r .. t(n) r + r - 1 of u.
//   Rounding rule of u (vlr_decoder_layer_fwd_lora_ex: lora_group_a -> lora_rows.hip / vlr_gemm_bf16_scaled): the fp32 sum of x A^T is
//   multiplied by scale = lora_alpha / r in fp32 and rounded ONCE to bf16; the B half then reads bf16 u and accumulates in fp32.
// Two steps, no atomics, every sum in a fixed order:
//   1. gemv_kernel itself on A (N = targets * r): the fp32 split-K partials of x A^T go to the caller's `u` scratch
//   2. the main launch gets ONE more K slice: workgroups with blockIdx.y == S fold those partials in slice order, scale, round to bf16
//      (LDS) and write  sum_j u[m][t(n) r + j] B[n][j]  (j ascending, plain FMAs - 16 x r x 64 of them per workgroup, against the
//      64 x K / S MACs of a base workgroup) as partial slice S.  gemv_epilogue_kernel sums slices 0 .. S in order, so the adapter term is
//      in the fp32 accumulator BEFORE bias / RoPE / SwiGLU / residual, and is added last: B = 0 gives acc + 0.0f = acc, bit for bit.
// The same slice rides the packed kernel (gemv_w4_lora_kernel, 128 columns per workgroup).
struct GemvLora {
    const float* upart;      // [Su][M][R] fp32 partials of x A^T
    const bf16_t* B;         // [N][r]
    int Su, r, R, targets;   // R = targets * r
    int n1, n2, n3;          // target t owns rows [n_t, n_t+1): n0 = 0, n1, n2, n3 (= N from the last target on)
    float scale;
};
__device__ __forceinline__ int lora_target(const GemvLora& lo, int n) { return (n >= lo.n1) + (n >= lo.n2) + (n >= lo.n3); }

// COLS output columns from n0 on; ub: COLS * 256 bytes of LDS = 16 rows x COLS * 8 bf16 columns of u.  The column block spans the
// targets t_lo .. t_hi (one, or two where a target edge falls inside it); the rank is walked in chunks of RC columns per spanned target
// so that any r fits (one chunk whenever (t_hi - t_lo + 1) * r <= COLS * 8: every shipped configuration); j stays ascending across chunks
// The 16 rows are rows mbase .. mbase + M - 1 of the call's Mtot (the wide form walks its row tiles; the 16-row calls pass M, 0)
template <int COLS>
__device__ __forceinline__ void gemv_lora_slice(const GemvLora& lo, float* __restrict__ slice, int M, int N, int n0, bf16_t* ub, int Mtot,
                                                int mbase) {
    constexpr int RP = 16 * COLS / 256;                      // rows of m per thread
    constexpr int CAP = COLS * 8;                            // bf16 columns of u per row the LDS holds
    const int nlast = min(n0 + COLS, N) - 1;
    const int t_lo = lora_target(lo, n0), nt = lora_target(lo, nlast) - t_lo + 1;      // nt <= 4 (host: targets <= 4)
    const int RC = min(lo.r, CAP / nt / 8 * 8), Wd = nt * RC;
    const int col = threadIdx.x % COLS, m0 = (threadIdx.x / COLS) * RP, n = n0 + col;
    const bool nok = n < N;
    const bf16_t* brow = lo.B + (size_t)(nok ? n : 0) * lo.r;
    const bf16_t* urow = ub + (nok ? lora_target(lo, n) - t_lo : 0) * RC;
    float acc[RP];
#pragma unroll
    for (int i = 0; i < RP; ++i) acc[i] = 0.f;
    for (int jc = 0; jc < lo.r; jc += RC) {
        const int rc = min(RC, lo.r - jc);                   // a multiple of 8
        if (jc) __syncthreads();                             // the previous chunk has been read
        for (int idx = threadIdx.x; idx < M * nt * rc; idx += 256) {
            const int m = idx / (nt * rc), c = idx % (nt * rc), tt = c / rc, j = c % rc;
            float s = 0.f;
            for (int k = 0; k < lo.Su; ++k) s += lo.upart[((size_t)k * Mtot + mbase + m) * lo.R + (t_lo + tt) * lo.r + jc + j];     // split order: fixed
            ub[m * Wd + tt * RC + j] = f32_to_bf16(lo.scale * s);
        }
        __syncthreads();
        if (!nok) continue;
        for (int j0 = 0; j0 < rc; j0 += 8) {
            float bf[8];
            unpack8(*reinterpret_cast<const u32x4*>(brow + jc + j0), bf);
#pragma unroll
            for (int i = 0; i < RP; ++i) {
                if (m0 + i >= M) continue;
                float uf[8];
                unpack8(*reinterpret_cast<const u32x4*>(urow + (m0 + i) * Wd + j0), uf);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[i] = __builtin_fmaf(uf[e], bf[e], acc[i]);
            }
        }
    }
    if (!nok) return;
#pragma unroll
    for (int i = 0; i < RP; ++i)
        if (m0 + i < M) slice[(size_t)(mbase + m0 + i) * N + n] = acc[i];
}

// grid (column blocks, S + 1): slices 0 .. S - 1 are gemv_kernel's, slice S the adapter term
__global__ __launch_bounds__(256) void gemv_lora_kernel(const bf16_t* __restrict__ X, int ldx, const bf16_t* __restrict__ W,
                                                        float* __restrict__ part, int M, int N, int K, int cps, int S, GemvLora lo) {
    __shared__ float red[4][16][GV_COLS];
    if ((int)blockIdx.y == S) gemv_lora_slice<GV_COLS>(lo, part + (size_t)S * M * N, M, N, blockIdx.x * GV_COLS, (bf16_t*)&red[0][0][0], M, 0);
    else gemv_tile<1>(X, ldx, W, part, M, N, K, cps, blockIdx.x * GV_COLS, blockIdx.y, red);
}

// the wide form: the adapter slice walks the row tiles through the 16-row code (per row: the same rank chunks, j ascending, u rounded once)
template <int MT>
__global__ __launch_bounds__(256) void gemv_wide_lora_kernel(const bf16_t* __restrict__ X, int ldx, const bf16_t* __restrict__ W,
                                                             float* __restrict__ part, int M, int N, int K, int cps, int S, GemvLora lo) {
    __shared__ float red[4][16][GV_COLS];
    if ((int)blockIdx.y == S) {
        for (int mt = 0; mt < MT; ++mt) {
            if (mt) __syncthreads();                       // the previous tile's u has been read
            gemv_lora_slice<GV_COLS>(lo, part + (size_t)S * M * N, min(16, M - 16 * mt), N, blockIdx.x * GV_COLS, (bf16_t*)&red[0][0][0], M,
                                     16 * mt);
        }
    } else gemv_tile<MT>(X, ldx, W, part, M, N, K, cps, blockIdx.x * GV_COLS, blockIdx.y, red);
}

struct GemvEpi {
    int mode;
    const float* part;
    int S, M, N;
    void* Y;
    int ldy;
    const bf16_t* bias;
    const void* res;
    int ldr;
    const int* pos;
    const float* cos_t;
    const float* sin_t;
    int rope_cols, hd, max_pos;
};

__device__ __forceinline__ float gv_acc(const GemvEpi& p, int m, int n) {
    float s = 0.f;
    for (int k = 0; k < p.S; ++k) s += p.part[((size_t)k * p.M + m) * p.N + n];     // split order: fixed
    return s;
}

// one thread = one output element (one rotated pair under RoPE): consecutive threads read consecutive partials, and M x N threads fill
// the chip even at M = 1 (an 8-column-per-thread form ran on 8 workgroups at M = 4, N = 4096 and took ~15 us per call)
__global__ __launch_bounds__(256) void gemv_epilogue_kernel(GemvEpi p, int units) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= p.M * units) return;
    const int m = gid / units, u = gid % units;
    if (p.mode == VLR_GEMV_SWIGLU) {                          // N = 2 I: gate columns [0, I), up columns [I, 2 I)
        const int I = p.N / 2;
        const float gt = gv_acc(p, m, u), up = gv_acc(p, m, I + u);
        ((bf16_t*)p.Y)[(size_t)m * p.ldy + u] = f32_to_bf16(gt * fast_sigmoid(gt) * up);
        return;
    }
    if (p.mode == VLR_GEMV_QKV_ROPE) {
        const int half = p.hd / 2;
        bf16_t* y = (bf16_t*)p.Y + (size_t)m * p.ldy;
        if (u < p.rope_cols / 2) {                            // frequency f of one rotated head: columns c1 and c1 + hd / 2
            const int head = u / half, f = u % half;
            const int c1 = head * p.hd + f, c2 = c1 + half;
            int ps = p.pos[m];
            ps = ps < 0 ? 0 : (ps >= p.max_pos ? p.max_pos - 1 : ps);
            float x1 = gv_acc(p, m, c1), x2 = gv_acc(p, m, c2);
            if (p.bias) { x1 += bf16_to_f32(p.bias[c1]); x2 += bf16_to_f32(p.bias[c2]); }
            const float cs = p.cos_t[(size_t)ps * half + f], sn = p.sin_t[(size_t)ps * half + f];
            y[c1] = f32_to_bf16(x1 * cs - x2 * sn);
            y[c2] = f32_to_bf16(x2 * cs + x1 * sn);
            return;
        }
        const int c = p.rope_cols + u - p.rope_cols / 2;
        y[c] = f32_to_bf16(gv_acc(p, m, c) + (p.bias ? bf16_to_f32(p.bias[c]) : 0.f));
        return;
    }
    float v = gv_acc(p, m, u) + (p.bias ? bf16_to_f32(p.bias[u]) : 0.f);
    if (p.mode == VLR_GEMV_BF16) {
        if (p.res) v += bf16_to_f32(((const bf16_t*)p.res)[(size_t)m * p.ldr + u]);
        ((bf16_t*)p.Y)[(size_t)m * p.ldy + u] = f32_to_bf16(v);
    } else {                                                  // fp32 out (VLR_GEMV_F32), + fp32 residual (VLR_GEMV_F32RES, in place allowed)
        if (p.mode == VLR_GEMV_F32RES && p.res) v += ((const float*)p.res)[(size_t)m * p.ldr + u];
        ((float*)p.Y)[(size_t)m * p.ldy + u] = v;
    }
}

// split count: enough workgroups for the chip, every split at least one chunk per wave where K allows
static int gemv_splits(int N, int K, int cols = GV_COLS) {
    const int nb = (N + cols - 1) / cols, nchunks = (K + GV_CHUNK - 1) / GV_CHUNK;
    int s = (GV_TARGET_WGS + nb - 1) / nb;
    const int smax = (nchunks + 3) / 4;
    s = s < 1 ? 1 : (s > smax ? smax : s);
    const int cps = (nchunks + s - 1) / s;
    return (nchunks + cps - 1) / cps;                         // no empty split
}

__global__ __launch_bounds__(256) void kv_cache_write_kernel(const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int ld,
                                                             bf16_t* __restrict__ kc, bf16_t* __restrict__ vc, int S, int kvh, int hd,
                                                             int cap, int slot0, long per) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * per) return;
    const bool isv = i >= per;
    if (isv) i -= per;
    const int v8 = hd / 8;
    const int e8 = (int)(i % v8);
    long rest = i / v8;
    const int h = (int)(rest % kvh);
    rest /= kvh;
    const int s = (int)(rest % S);
    const long b = rest / S;
    const bf16_t* src = (isv ? v : k) + (size_t)(b * S + s) * ld + (size_t)h * hd + e8 * 8;
    bf16_t* dst = (isv ? vc : kc) + (((size_t)b * kvh + h) * cap + slot0 + s) * hd + e8 * 8;
    *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
}

constexpr int AD_HD = 128;
constexpr int AD_REC = 132;          // floats per (sequence, head, chunk) partial: max, sum, 2 pad, accumulator [128]
constexpr int AD_CMAX = 256, AD_CMIN = 64;
constexpr int AD_TARGET_WGS = 1024;

static int attn_decode_chunk(int B, int kvh, int len) {
    int C = AD_CMAX;
    while (C > AD_CMIN && (long)B * kvh * ((len + C - 1) / C) < AD_TARGET_WGS) C /= 2;
    return C;
}

// grid (chunk, kv head, sequence), 256 threads.  Scores in the log2 domain (scale * log2 e folded into q . k).
// key_mask == nullptr (the tail segment of vlr_attn_decode_shared): all `len` columns are attended.
template <int G>
__global__ __launch_bounds__(256) void attn_decode_kernel(const bf16_t* __restrict__ q, int ldq, const bf16_t* __restrict__ kc,
                                                          const bf16_t* __restrict__ vc, const int* __restrict__ key_mask,
                                                          float* __restrict__ ws, int kvh, int cap, int len, int C, int nchunks,
                                                          float sl2) {
    __shared__ float sc[G][AD_CMAX];
    __shared__ float red[4][G][AD_HD];
    const int c = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, d0 = (lane & 15) * 8;
    const int j0 = c * C;
    const bf16_t* kbase = kc + ((size_t)b * kvh + hk) * cap * AD_HD;
    const bf16_t* vbase = vc + ((size_t)b * kvh + hk) * cap * AD_HD;
    const int* km = key_mask ? key_mask + (size_t)b * cap : nullptr;      // null: every column below len is attended
    float qf[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) unpack8(*reinterpret_cast<const u32x4*>(q + (size_t)b * ldq + (size_t)(hk * G + g) * AD_HD + d0), qf[g]);
    // ---- scores: 16 lanes per key (8 dims each), 4 keys per wave-instruction, 4 keys in flight per lane
    for (int i0 = wv * 4 + (lane >> 4); i0 < C; i0 += 64) {
        u32x4 kr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + i0 + 16 * u;
            kr[u] = j < len ? *reinterpret_cast<const u32x4*>(kbase + (size_t)j * AD_HD + d0) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float kf[8];
            unpack8(kr[u], kf);
            const int i = i0 + 16 * u, j = j0 + i;
            const bool valid = j < len && (!km || km[j] != 0);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) s += qf[g][e] * kf[e];
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
                if ((lane & 15) == 0) sc[g][i] = valid ? s * sl2 : -INFINITY;
            }
        }
    }
    __syncthreads();
    // ---- chunk softmax statistics: wave g % 4 owns query head g
    float* rec = ws + (((size_t)b * kvh + hk) * nchunks + c) * G * AD_REC;
    for (int g = wv; g < G; g += 4) {
        float mx = -INFINITY;
        for (int i = lane; i < C; i += 64) mx = fmaxf(mx, sc[g][i]);
        mx = wave_max(mx);
        float l = 0.f;
        for (int i = lane; i < C; i += 64) {
            const float pr = mx == -INFINITY ? 0.f : exp2f(sc[g][i] - mx);
            sc[g][i] = pr;
            l += pr;
        }
        l = wave_sum(l);
        if (lane == 0) { rec[g * AD_REC] = mx; rec[g * AD_REC + 1] = l; }
    }
    __syncthreads();
    // ---- P V: 16 lanes per key (8 dims each), 16 key groups; keys whose probabilities are all zero are skipped (masked, or beyond len)
    float o[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) o[g][e] = 0.f;
    const int kg = threadIdx.x >> 4;
    for (int i0 = kg; i0 < C; i0 += 64) {
        u32x4 vr[4];
        bool use[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + 16 * u;
            bool any = false;
#pragma unroll
            for (int g = 0; g < G; ++g) any |= sc[g][i] != 0.f;
            use[u] = any && j0 + i < len;
            vr[u] = use[u] ? *reinterpret_cast<const u32x4*>(vbase + (size_t)(j0 + i) * AD_HD + d0) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (!use[u]) continue;
            float vf[8];
            unpack8(vr[u], vf);
            const int i = i0 + 16 * u;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float pr = sc[g][i];
#pragma unroll
                for (int e = 0; e < 8; ++e) o[g][e] += pr * vf[e];
            }
        }
    }
    // the 4 key groups of a wave (lane bits 4, 5), then the 4 waves through LDS in wave order
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float x = o[g][e];
            x += __shfl_xor(x, 16);
            x += __shfl_xor(x, 32);
            o[g][e] = x;
        }
    if (lane < 16)
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int e = 0; e < 8; ++e) red[wv][g][d0 + e] = o[g][e];
    __syncthreads();
    for (int t = threadIdx.x; t < G * AD_HD; t += 256) {
        const int g = t / AD_HD, d = t % AD_HD;
        rec[g * AD_REC + 4 + d] = ((red[0][g][d] + red[1][g][d]) + red[2][g][d]) + red[3][g][d];
    }
}

// grid (heads, batch), 128 threads = one per feature; chunks folded in order
__global__ __launch_bounds__(128) void attn_decode_combine_kernel(const float* __restrict__ ws, bf16_t* __restrict__ o, int ldo, int heads,
                                                                  int kvh, int nchunks) {
    const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
    const int G = heads / kvh, hk = h / G, g = h % G;
    const float* base = ws + ((size_t)b * kvh + hk) * nchunks * G * AD_REC + (size_t)g * AD_REC;
    float mx = -INFINITY;
    for (int c = 0; c < nchunks; ++c) mx = fmaxf(mx, base[(size_t)c * G * AD_REC]);
    float l = 0.f, acc = 0.f;
    if (mx != -INFINITY)
        for (int c = 0; c < nchunks; ++c) {
            const float* rc = base + (size_t)c * G * AD_REC;
            const float m = rc[0];
            if (m == -INFINITY) continue;
            const float w = exp2f(m - mx);
            l += w * rc[1];
            acc += w * rc[4 + d];
        }
    o[(size_t)b * ldo + (size_t)h * AD_HD + d] = f32_to_bf16(l > 0.f ? acc / l : 0.f);
}

extern "C" long vlr_gemv_workspace_bytes(int M, int N, int K) {
    if (M < 1 || N < 1 || K < 8) return 0;
    return (long)gemv_splits(N, K) * (M > 16 ? 16 : M) * N * 4;
}

// the argument rules and the epilogue launch the bf16 and the packed skinny GEMM share
static int gemv_check(const char* fn, int mode, const void* X, int ldx, const void* Y, int ldy, const void* bias, const void* residual,
                      int ldr, const int* pos, const float* cos_t, const float* sin_t, int rope_cols, int head_dim, int max_pos, int M,
                      int N, int K, const void* workspace, int max_rows = 16) {
    VLR_REQUIRE(mode >= VLR_GEMV_BF16 && mode <= VLR_GEMV_SWIGLU, "%s: unknown mode %d", fn, mode);
    VLR_REQUIRE(X && Y && workspace, "%s: null argument", fn);
    VLR_REQUIRE(M >= 1 && M <= max_rows, "%s: M = %d rows, the skinny GEMM takes 1 <= M <= %d", fn, M, max_rows);
    VLR_REQUIRE(K >= 8 && K % 8 == 0, "%s: K = %d must be a positive multiple of 8", fn, K);
    VLR_REQUIRE(N >= 1 && ldx >= K && ldx % 8 == 0 && ((uintptr_t)X & 15) == 0, "%s: N %d, ldx %d (>= K, multiple of 8) and 16-byte aligned X required",
                fn, N, ldx);
    const int ncols = mode == VLR_GEMV_SWIGLU ? N / 2 : N;
    VLR_REQUIRE(ldy >= ncols, "%s: ldy %d < output columns %d", fn, ldy, ncols);
    VLR_REQUIRE(mode != VLR_GEMV_SWIGLU || N % 2 == 0, "%s: gate|up needs an even N (got %d)", fn, N);
    VLR_REQUIRE(mode == VLR_GEMV_BF16 || mode == VLR_GEMV_F32RES || !residual, "%s: mode %d takes no residual", fn, mode);
    VLR_REQUIRE(!residual || ldr >= N, "%s: ldr %d < N %d", fn, ldr, N);
    VLR_REQUIRE(!bias || mode == VLR_GEMV_BF16 || mode == VLR_GEMV_F32 || mode == VLR_GEMV_QKV_ROPE, "%s: mode %d takes no bias", fn, mode);
    if (mode == VLR_GEMV_QKV_ROPE)
        VLR_REQUIRE(pos && cos_t && sin_t && head_dim >= 16 && head_dim % 16 == 0 && rope_cols % head_dim == 0 && rope_cols >= 0 &&
                        rope_cols <= N && max_pos > 0,
                    "%s: RoPE needs pos / cos / sin tables, head_dim %d (multiple of 16), rope_cols %d (multiple of head_dim, <= N %d)", fn,
                    head_dim, rope_cols, N);
    return VLR_OK;
}

static void gemv_epilogue(int mode, const void* workspace, int S, void* Y, int ldy, const void* bias, const void* residual, int ldr,
                          const int* pos, const float* cos_t, const float* sin_t, int rope_cols, int head_dim, int max_pos, int M, int N,
                          hipStream_t st) {
    GemvEpi p{mode, (const float*)workspace, S, M, N, Y, ldy, (const bf16_t*)bias, residual, ldr, pos, cos_t, sin_t, rope_cols,
              head_dim, max_pos};
    const int units = mode == VLR_GEMV_SWIGLU ? N / 2 : (mode == VLR_GEMV_QKV_ROPE ? N - rope_cols / 2 : N);
    hipLaunchKernelGGL(gemv_epilogue_kernel, dim3((M * units + 255) / 256), dim3(256), 0, st, p, units);
}

// the product launch for any M <= 64: the 16-row kernel itself up to 16 rows, else one pass over W for all ceil(M / 16) row tiles
static void gemv_launch(dim3 grid, hipStream_t st, const void* X, int ldx, const void* W, void* part, int M, int N, int K, int cps) {
    const bf16_t* x = (const bf16_t*)X;
    const bf16_t* w = (const bf16_t*)W;
    float* p = (float*)part;
    switch ((M + 15) / 16) {
        case 1: hipLaunchKernelGGL(gemv_kernel, grid, dim3(256), 0, st, x, ldx, w, p, M, N, K, cps); break;
        case 2: hipLaunchKernelGGL(gemv_wide_kernel<2>, grid, dim3(256), 0, st, x, ldx, w, p, M, N, K, cps); break;
        case 3: hipLaunchKernelGGL(gemv_wide_kernel<3>, grid, dim3(256), 0, st, x, ldx, w, p, M, N, K, cps); break;
        default: hipLaunchKernelGGL(gemv_wide_kernel<4>, grid, dim3(256), 0, st, x, ldx, w, p, M, N, K, cps); break;
    }
}

static int gemv_bf16_rows(const char* fn, int max_rows, int mode, const void* X, int ldx, const void* W, void* Y, int ldy, const void* bias,
                          const void* residual, int ldr, const int* pos, const float* cos_t, const float* sin_t, int rope_cols, int head_dim,
                          int max_pos, int M, int N, int K, void* workspace, hipStream_t st) {
    const int rc = gemv_check(fn, mode, X, ldx, Y, ldy, bias, residual, ldr, pos, cos_t, sin_t, rope_cols, head_dim, max_pos, M, N, K,
                              workspace, max_rows);
    if (rc != VLR_OK) return rc;
    VLR_REQUIRE(W && ((uintptr_t)W & 15) == 0, "%s: W must be non-null and 16-byte aligned", fn);
    const int S = gemv_splits(N, K);
    const int nchunks = (K + GV_CHUNK - 1) / GV_CHUNK, cps = (nchunks + S - 1) / S;
    gemv_launch(dim3((N + GV_COLS - 1) / GV_COLS, S), st, X, ldx, W, workspace, M, N, K, cps);
    gemv_epilogue(mode, workspace, S, Y, ldy, bias, residual, ldr, pos, cos_t, sin_t, rope_cols, head_dim, max_pos, M, N, st);
    return vlr_check_launch(fn);
}

extern "C" int vlr_gemv_bf16(int mode, const void* X, int ldx, const void* W, void* Y, int ldy, const void* bias, const void* residual,
                             int ldr, const int* pos, const float* cos_t, const float* sin_t, int rope_cols, int head_dim, int max_pos,
                             int M, int N, int K, void* workspace, vlr_stream_t st) {
    return gemv_bf16_rows("vlr_gemv_bf16", 16, mode, X, ldx, W, Y, ldy, bias, residual, ldr, pos, cos_t, sin_t, rope_cols, head_dim, max_pos, M,
                          N, K, workspace, st);
}

// ---- the wide entry points: the argument lists of their 16-row namesakes, 1 <= M <= 64 rows in one pass over W.  Bit for bit the
// 16-row entry point on rows [0, 16), [16, 32), ... (gemv_tile).  Workspace: the same split count times min(M, 64) rows.
extern "C" long vlr_gemv_wide_workspace_bytes(int M, int N, int K) {
    if (M < 1 || N < 1 || K < 8) return 0;
    return (long)gemv_splits(N, K) * (M > 64 ? 64 : M) * N * 4;
}
extern "C" int vlr_gemv_wide_bf16(int mode, const void* X, int ldx, const void* W, void* Y, int ldy, const void* bias, const void* residual,
                                  int ldr, const int* pos, const float* cos_t, const float* sin_t, int rope_cols, int head_dim, int max_pos,
                                  int M, int N, int K, void* workspace, vlr_stream_t st) {
    return gemv_bf16_rows("vlr_gemv_wide_bf16", 64, mode, X, ldx, W, Y, ldy, bias, residual, ldr, pos, cos_t, sin_t, rope_cols, head_dim,
                          max_pos, M, N, K, workspace, st);
}

// ---- the adapter entry points.  Workspace: one more fp32 slice than the adapter-free call; u scratch: the split-K partials of x A^T
extern "C" long vlr_gemv_lora_u_bytes(int M, int K, int r_total) { return vlr_gemv_workspace_bytes(M, r_total, K); }
extern "C" long vlr_gemv_lora_workspace_bytes(int M, int N, int K, int r_total) {
    if (M < 1 || N < 1 || K < 8 || r_total < 8 || r_total % 8) return 0;
    const int s = gemv_splits(N, K), s4 = gemv_splits(N, K, 2 * GV_COLS);       // bf16 and packed (GW_COLS = 128) split counts
    return (long)((s > s4 ? s : s4) + 1) * (M > 16 ? 16 : M) * N * 4;
}
// checks the adapter arguments, launches step 1 (x A^T partials -> u) and fills `lo`
static int gemv_lora_prepare(const char* fn, const void* X, int ldx, const void* A, const void* B, int r, int targets, const int* outs,
                             float scale, void* u, int M, int N, int K, hipStream_t st, GemvLora* lo) {
    VLR_REQUIRE(A && B && u, "%s: null adapter argument (A, B and the u scratch are needed; pass A = B = NULL for no adapter)", fn);
    VLR_REQUIRE(r >= 8 && r % 8 == 0, "%s: LoRA rank %d must be a positive multiple of 8", fn, r);
    VLR_REQUIRE(targets >= 1 && targets <= 4, "%s: targets %d outside 1 .. 4", fn, targets);
    VLR_REQUIRE((((uintptr_t)A | (uintptr_t)B | (uintptr_t)u) & 15) == 0, "%s: A, B and u must be 16-byte aligned", fn);
    int edge[5] = {0, N, N, N, N};
    if (outs) {
        for (int t = 0; t < targets; ++t) {
            VLR_REQUIRE(outs[t] >= 1, "%s: target %d has %d rows", fn, t, outs[t]);
            edge[t + 1] = edge[t] + outs[t];
        }
        VLR_REQUIRE(edge[targets] == N, "%s: the targets' rows sum to %d, N is %d", fn, edge[targets], N);
    } else {
        VLR_REQUIRE(N % targets == 0, "%s: N %d is not a multiple of targets %d (pass the row split)", fn, N, targets);
        for (int t = 0; t < targets; ++t) edge[t + 1] = edge[t] + N / targets;
    }
    for (int t = targets; t < 4; ++t) edge[t + 1] = N;
    const int R = targets * r, Su = gemv_splits(R, K);
    const int nchunks = (K + GV_CHUNK - 1) / GV_CHUNK, cps = (nchunks + Su - 1) / Su;
    gemv_launch(dim3((R + GV_COLS - 1) / GV_COLS, Su), st, X, ldx, A, u, M, R, K, cps);
    *lo = GemvLora{(const float*)u, (const bf16_t*)B, Su, r, R, targets, edge[1], edge[2], edge[3], scale};      // edge[targets] = N: no row beyond it
    return VLR_OK;
}

static int gemv_bf16_lora_rows(const char* fn, int max_rows, int mode, const void* X, int ldx, const void* W, void* Y, int ldy,
                               const void* bias, const void* residual, int ldr, const int* pos, const float* cos_t, const float* sin_t,
                               int rope_cols, int head_dim, int max_pos, int M, int N, int K, void* workspace, const void* A, const void* B,
                               int r, int targets, const int* outs, float scale, void* u, hipStream_t st) {
    const int rc = gemv_check(fn, mode, X, ldx, Y, ldy, bias, residual, ldr, pos, cos_t, sin_t, rope_cols, head_dim, max_pos, M, N, K,
                              workspace, max_rows);
    if (rc != VLR_OK) return rc;
    VLR_REQUIRE(W && ((uintptr_t)W & 15) == 0, "%s: W must be non-null and 16-byte aligned", fn);
    GemvLora lo;
    const int rl = gemv_lora_prepare(fn, X, ldx, A, B, r, targets, outs, scale, u, M, N, K, st, &lo);
    if (rl != VLR_OK) return rl;
    const int S = gemv_splits(N, K);
    const int nchunks = (K + GV_CHUNK - 1) / GV_CHUNK, cps = (nchunks + S - 1) / S;
    const dim3 grid((N + GV_COLS - 1) / GV_COLS, S + 1);
    const bf16_t* x = (const bf16_t*)X;
    const bf16_t* w = (const bf16_t*)W;
    float* p = (float*)workspace;
    switch ((M + 15) / 16) {
        case 1: hipLaunchKernelGGL(gemv_lora_kernel, grid, dim3(256), 0, st, x, ldx, w, p, M, N, K, cps, S, lo); break;
        case 2: hipLaunchKernelGGL(gemv_wide_lora_kernel<2>, grid, dim3(256), 0, st, x, ldx, w, p, M, N, K, cps, S, lo); break;
        case 3: hipLaunchKernelGGL(gemv_wide_lora_kernel<3>, grid, dim3(256), 0, st, x, ldx, w, p, M, N, K, cps, S, lo); break;
        default: hipLaunchKernelGGL(gemv_wide_lora_kernel<4>, grid, dim3(256), 0, st, x, ldx, w, p, M, N, K, cps, S, lo); break;
    }
    gemv_epilogue(mode, workspace, S + 1, Y, ldy, bias, residual, ldr, pos, cos_t, sin_t, rope_cols, head_dim, max_pos, M, N, st);
    return vlr_check_launch(fn);
}

extern "C" int vlr_gemv_bf16_lora(int mode, const void* X, int ldx, const void* W, void* Y, int ldy, const void* bias, const void* residual,
                                  int ldr, const int* pos, const float* cos_t, const float* sin_t, int rope_cols, int head_dim, int max_pos,
                                  int M, int N, int K, void* workspace, const void* A, const void* B, int r, int targets, const int* outs,
                                  float scale, void* u, vlr_stream_t st) {
    if (!A && !B)      // not adapted: the adapter-free call itself
        return vlr_gemv_bf16(mode, X, ldx, W, Y, ldy, bias, residual, ldr, pos, cos_t, sin_t, rope_cols, head_dim, max_pos, M, N, K, workspace, st);
    return gemv_bf16_lora_rows("vlr_gemv_bf16_lora", 16, mode, X, ldx, W, Y, ldy, bias, residual, ldr, pos, cos_t, sin_t, rope_cols, head_dim,
                               max_pos, M, N, K, workspace, A, B, r, targets, outs, scale, u, st);
}

// the wide adapter call: x A^T is the wide kernel on A, the adapter slice walks the row tiles (gemv_wide_lora_kernel)
extern "C" long vlr_gemv_wide_lora_u_bytes(int M, int K, int r_total) { return vlr_gemv_wide_workspace_bytes(M, r_total, K); }
extern "C" long vlr_gemv_wide_lora_workspace_bytes(int M, int N, int K, int r_total) {
    if (M < 1 || N < 1 || K < 8 || r_total < 8 || r_total % 8) return 0;
    const int s = gemv_splits(N, K), s4 = gemv_splits(N, K, 2 * GV_COLS);       // vlr_gemv_lora_workspace_bytes' rule: equal to it at M <= 16
    return (long)((s > s4 ? s : s4) + 1) * (M > 64 ? 64 : M) * N * 4;
}
extern "C" int vlr_gemv_wide_bf16_lora(int mode, const void* X, int ldx, const void* W, void* Y, int ldy, const void* bias,
                                       const void* residual, int ldr, const int* pos, const float* cos_t, const float* sin_t, int rope_cols,
                                       int head_dim, int max_pos, int M, int N, int K, void* workspace, const void* A, const void* B, int r,
                                       int targets, const int* outs, float scale, void* u, vlr_stream_t st) {
    if (!A && !B)
        return vlr_gemv_wide_bf16(mode, X, ldx, W, Y, ldy, bias, residual, ldr, pos, cos_t, sin_t, rope_cols, head_dim, max_pos, M, N, K,
                                  workspace, st);
    return gemv_bf16_lora_rows("vlr_gemv_wide_bf16_lora", 64, mode, X, ldx, W, Y, ldy, bias, residual, ldr, pos, cos_t, sin_t, rope_cols,
                               head_dim, max_pos, M, N, K, workspace, A, B, r, targets, outs, scale, u, st);
}

// ---- the skinny GEMM over packed int4 weights.  A workgroup owns 128 output columns (two halves of 64) and one K slice.  Lane (r, g)
// of a 32-k step holds the X fragment A[m = r][k = 8 g + j] and, per half h, ONE 16-byte load of qweight row k / 8: the words of columns
// n0 + 64 h + 4 r + t, t = 0 .. 3.  MFMA n tile (h, t) is therefore the 16 columns {n0 + 64 h + 4 r + t}: the tiles interleave, every load
// is 16 bytes and a wave reads 4 rows x 256 contiguous bytes per instruction.  PER_STEP: the group size is below the 128-k chunk, so
// scales and zeros are reloaded at every 32-k step (a multiple of 32 divides the step into one group); otherwise once per chunk.
constexpr int GW_COLS = 128;

// MT row tiles of 16 (M <= 16 MT): a lane's packed words are unpacked ONCE per (k step, half, n tile) and the fragment feeds MT MFMAs,
// so the unpack - what bounds the 16-row kernel - is shared by up to 64 rows; only the X fragments and the accumulators grow
// with MT.  Row m = 16 mt + r sees the chunks, the k steps and the four-wave fold of the MT = 1 form in the same order: its sums do not
// depend on MT.  The fold runs one row tile at a time through the same 32 KB of LDS.
template <bool PER_STEP, int MT>
__device__ __forceinline__ void gemv_w4_tile(const bf16_t* __restrict__ X, int ldx, const uint32_t* __restrict__ QW,
                                             const uint32_t* __restrict__ QZ, const uint16_t* __restrict__ SC, float* __restrict__ part,
                                             int M, int N, int K, int gsz, int cps, int n0, int split, float (*red)[16][GW_COLS]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int nchunks = (K + GV_CHUNK - 1) / GV_CHUNK;
    const int c0 = split * cps, c1 = min(nchunks, c0 + cps);
    bool mok[MT];
    const bf16_t* xrow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        mok[mt] = 16 * mt + r < M;
        xrow[mt] = X + (size_t)(mok[mt] ? 16 * mt + r : 0) * ldx;
    }
    int nb[2];
    bool nok[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int n = n0 + 64 * h + 4 * r;
        nok[h] = n < N;                                    // N % 8 == 0: a lane's 4 columns are all in or all out
        nb[h] = nok[h] ? n : 0;
    }
    f32x4 acc[MT][2][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[mt][h][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bf16x8 zero = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
    const int nz = N / 8, lastk = K - 8;
    constexpr int NS = PER_STEP ? 4 : 1;
    // every load below is unconditional at a clamped address (no branch, all of a chunk's loads in flight together): a k beyond K reads
    // row K / 8 - 1 again and meets X = 0, a column beyond N reads column 0 and is never stored, a row beyond M reads row 0 and is zeroed
    for (int c = c0 + wv; c < c1; c += 4) {
        f16x4 sc[NS][2];
        uint32_t zw[NS][2];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int G = min(c * GV_CHUNK + s * 32, lastk) / gsz;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                sc[s][h] = __builtin_bit_cast(f16x4, *reinterpret_cast<const u32x2*>(SC + (size_t)G * N + nb[h]));
                zw[s][h] = QZ[(size_t)G * nz + (nb[h] >> 3)];
            }
        }
        bf16x8 a[4][MT];
        u32x4 qw[4][2];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = c * GV_CHUNK + u * 32 + g * 8;
            const int kc = min(k, lastk);                  // K % 8 == 0: a lane's 8 k are all in or all out
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const bf16x8 x = load8(xrow[mt] + kc);
                a[u][mt] = (mok[mt] && k < K) ? x : zero;
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) qw[u][h] = *reinterpret_cast<const u32x4*>(QW + (size_t)(kc >> 3) * N + nb[h]);
        }
        __builtin_amdgcn_sched_barrier(0);                 // every load of the chunk is issued before the first unpack waits on one
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int s = PER_STEP ? u : 0;
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const bf16x8 b = __builtin_bit_cast(bf16x8, w4_unpack(qw[u][h][t], (float)sc[s][h][t], w4_zero(zw[s][h], nb[h] + t)));
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
                        acc[mt][h][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u][mt], b, acc[mt][h][t], 0, 0, 0);
                }
        }
    }
    // D map: lane holds D[m = 16 mt + 4 g + i][tile column r] of n tile (h, t) = output column 64 h + 4 r + t
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        if (mt) __syncthreads();                           // the previous row tile has been folded
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) red[wv][4 * g + i][64 * h + 4 * r + t] = acc[mt][h][t][i];
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int idx = threadIdx.x + 256 * e, ml = idx / GW_COLS, m = 16 * mt + ml, n = idx % GW_COLS;
            if (m < M && n0 + n < N)
                part[((size_t)split * M + m) * N + n0 + n] = ((red[0][ml][n] + red[1][ml][n]) + red[2][ml][n]) + red[3][ml][n];
        }
    }
}

// MT = 1: the 16-row kernel; MT = 2 .. 4: the wide form (17 .. 64 rows in ONE pass over the packed words).  Grid, chunk assignment and
// partial layout [slice][M][N] do not depend on MT
template <bool PER_STEP, int MT = 1>
__global__ __launch_bounds__(256) void gemv_w4_kernel(const bf16_t* __restrict__ X, int ldx, const uint32_t* __restrict__ QW,
                                                      const uint32_t* __restrict__ QZ, const uint16_t* __restrict__ SC,
                                                      float* __restrict__ part, int M, int N, int K, int gsz, int cps) {
    __shared__ float red[4][16][GW_COLS];
    gemv_w4_tile<PER_STEP, MT>(X, ldx, QW, QZ, SC, part, M, N, K, gsz, cps, blockIdx.x * GW_COLS, blockIdx.y, red);
}

// the packed product with the adapter term as slice S (gemv_lora_kernel's scheme; the adapter operands are bf16 here too).  MT > 1: the
// adapter slice walks the row tiles through the 16-row code, as gemv_wide_lora_kernel does
template <bool PER_STEP, int MT = 1>
__global__ __launch_bounds__(256) void gemv_w4_lora_kernel(const bf16_t* __restrict__ X, int ldx, const uint32_t* __restrict__ QW,
                                                           const uint32_t* __restrict__ QZ, const uint16_t* __restrict__ SC,
                                                           float* __restrict__ part, int M, int N, int K, int gsz, int cps, int S,
                                                           GemvLora lo) {
    __shared__ float red[4][16][GW_COLS];
    if ((int)blockIdx.y == S) {
        for (int mt = 0; mt < MT; ++mt) {
            if (mt) __syncthreads();                       // the previous tile's u has been read
            gemv_lora_slice<GW_COLS>(lo, part + (size_t)S * M * N, min(16, M - 16 * mt), N, blockIdx.x * GW_COLS, (bf16_t*)&red[0][0][0], M,
                                     16 * mt);
        }
    } else gemv_w4_tile<PER_STEP, MT>(X, ldx, QW, QZ, SC, part, M, N, K, gsz, cps, blockIdx.x * GW_COLS, blockIdx.y, red);
}

static int gemv_w4_check(const char* fn, const void* qweight, const void* qzeros, const void* scales, int group_size, int N, int K) {
    VLR_REQUIRE(qweight && qzeros && scales, "%s: null packed weights", fn);
    VLR_REQUIRE(N % 8 == 0, "%s: N = %d must be a multiple of 8 (qzeros packs 8 columns per word)", fn, N);
    VLR_REQUIRE(group_size == K || (group_size >= 32 && group_size % 32 == 0 && K % group_size == 0),
                "%s: group_size %d must be K (%d) or a multiple of 32 that divides it", fn, group_size, K);
    VLR_REQUIRE(((uintptr_t)qweight & 15) == 0 && ((uintptr_t)scales & 7) == 0 && ((uintptr_t)qzeros & 3) == 0,
                "%s: qweight must be 16-byte, scales 8-byte, qzeros 4-byte aligned", fn);
    return VLR_OK;
}

extern "C" long vlr_gemv_w4_workspace_bytes(int M, int N, int K) {
    if (M < 1 || N < 1 || K < 8) return 0;
    return (long)gemv_splits(N, K, GW_COLS) * (M > 16 ? 16 : M) * N * 4;
}

// the product launch for any M <= 64: ceil(M / 16) row tiles; one scale / zero group per 128-k chunk when the chunks do not straddle
// groups, else per 32-k step (a group of K itself never changes)
static void gemv_w4_launch(dim3 grid, hipStream_t st, const void* X, int ldx, const void* qweight, const void* qzeros, const void* scales,
                           int group_size, void* part, int M, int N, int K, int cps, int S, const GemvLora* lo) {
    const bf16_t* x = (const bf16_t*)X;
    const uint32_t* qw = (const uint32_t*)qweight;
    const uint32_t* qz = (const uint32_t*)qzeros;
    const uint16_t* sc = (const uint16_t*)scales;
    float* p = (float*)part;
    const bool per_step = !(group_size == K || group_size % GV_CHUNK == 0);
#define W4_LAUNCH(PS, MT)                                                                                                          \
    do {                                                                                                                           \
        if (lo) hipLaunchKernelGGL((gemv_w4_lora_kernel<PS, MT>), grid, dim3(256), 0, st, x, ldx, qw, qz, sc, p, M, N, K, group_size, cps, S, *lo); \
        else hipLaunchKernelGGL((gemv_w4_kernel<PS, MT>), grid, dim3(256), 0, st, x, ldx, qw, qz, sc, p, M, N, K, group_size, cps);  \
    } while (0)
#define W4_ROWS(MT)                                                                                                                \
    do {                                                                                                                           \
        if (per_step) W4_LAUNCH(true, MT);                                                                                         \
        else W4_LAUNCH(false, MT);                                                                                                 \
    } while (0)
    switch ((M + 15) / 16) {
        case 1: W4_ROWS(1); break;
        case 2: W4_ROWS(2); break;
        case 3: W4_ROWS(3); break;
        default: W4_ROWS(4); break;
    }
#undef W4_ROWS
#undef W4_LAUNCH
}

static int gemv_w4_rows(const char* fn, int max_rows, int mode, const void* X, int ldx, const void* qweight, const void* qzeros,
                        const void* scales, int group_size, void* Y, int ldy, const void* bias, const void* residual, int ldr, const int* pos,
                        const float* cos_t, const float* sin_t, int rope_cols, int head_dim, int max_pos, int M, int N, int K,
                        void* workspace, hipStream_t st) {
    const int rc = gemv_check(fn, mode, X, ldx, Y, ldy, bias, residual, ldr, pos, cos_t, sin_t, rope_cols, head_dim, max_pos, M, N, K,
                              workspace, max_rows);
    if (rc != VLR_OK) return rc;
    const int rq = gemv_w4_check(fn, qweight, qzeros, scales, group_size, N, K);
    if (rq != VLR_OK) return rq;
    const int S = gemv_splits(N, K, GW_COLS);
    const int nchunks = (K + GV_CHUNK - 1) / GV_CHUNK, cps = (nchunks + S - 1) / S;
    gemv_w4_launch(dim3((N + GW_COLS - 1) / GW_COLS, S), st, X, ldx, qweight, qzeros, scales, group_size, workspace, M, N, K, cps, S, nullptr);
    gemv_epilogue(mode, workspace, S, Y, ldy, bias, residual, ldr, pos, cos_t, sin_t, rope_cols, head_dim, max_pos, M, N, st);
    return vlr_check_launch(fn);
}

static int gemv_w4_lora_rows(const char* fn, int max_rows, int mode, const void* X, int ldx, const void* qweight, const void* qzeros,
                             const void* scales, int group_size, void* Y, int ldy, const void* bias, const void* residual, int ldr,
                             const int* pos, const float* cos_t, const float* sin_t, int rope_cols, int head_dim, int max_pos, int M, int N,
                             int K, void* workspace, const void* A, const void* B, int r, int targets, const int* outs, float scale, void* u,
                             hipStream_t st) {
    const int rc = gemv_check(fn, mode, X, ldx, Y, ldy, bias, residual, ldr, pos, cos_t, sin_t, rope_cols, head_dim, max_pos, M, N, K,
                              workspace, max_rows);
    if (rc != VLR_OK) return rc;
    const int rq = gemv_w4_check(fn, qweight, qzeros, scales, group_size, N, K);
    if (rq != VLR_OK) return rq;
    GemvLora lo;
    const int rl = gemv_lora_prepare(fn, X, ldx, A, B, r, targets, outs, scale, u, M, N, K, st, &lo);
    if (rl != VLR_OK) return rl;
    const int S = gemv_splits(N, K, GW_COLS);
    const int nchunks = (K + GV_CHUNK - 1) / GV_CHUNK, cps = (nchunks + S - 1) / S;
    gemv_w4_launch(dim3((N + GW_COLS - 1) / GW_COLS, S + 1), st, X, ldx, qweight, qzeros, scales, group_size, workspace, M, N, K, cps, S, &lo);
    gemv_epilogue(mode, workspace, S + 1, Y, ldy, bias, residual, ldr, pos, cos_t, sin_t, rope_cols, head_dim, max_pos, M, N, st);
    return vlr_check_launch(fn);
}

extern "C" int vlr_gemv_w4(int mode, const void* X, int ldx, const void* qweight, const void* qzeros, const void* scales, int group_size,
                           void* Y, int ldy, const void* bias, const void* residual, int ldr, const int* pos, const float* cos_t,
                           const float* sin_t, int rope_cols, int head_dim, int max_pos, int M, int N, int K, void* workspace,
                           vlr_stream_t st) {
    return gemv_w4_rows("vlr_gemv_w4", 16, mode, X, ldx, qweight, qzeros, scales, group_size, Y, ldy, bias, residual, ldr, pos, cos_t, sin_t,
                        rope_cols, head_dim, max_pos, M, N, K, workspace, st);
}

extern "C" int vlr_gemv_w4_lora(int mode, const void* X, int ldx, const void* qweight, const void* qzeros, const void* scales, int group_size,
                                void* Y, int ldy, const void* bias, const void* residual, int ldr, const int* pos, const float* cos_t,
                                const float* sin_t, int rope_cols, int head_dim, int max_pos, int M, int N, int K, void* workspace,
                                const void* A, const void* B, int r, int targets, const int* outs, float scale, void* u, vlr_stream_t st) {
    if (!A && !B)
        return vlr_gemv_w4(mode, X, ldx, qweight, qzeros, scales, group_size, Y, ldy, bias, residual, ldr, pos, cos_t, sin_t, rope_cols,
                           head_dim, max_pos, M, N, K, workspace, st);
    return gemv_w4_lora_rows("vlr_gemv_w4_lora", 16, mode, X, ldx, qweight, qzeros, scales, group_size, Y, ldy, bias, residual, ldr, pos,
                             cos_t, sin_t, rope_cols, head_dim, max_pos, M, N, K, workspace, A, B, r, targets, outs, scale, u, st);
}

// ---- the wide packed entry points: the argument lists of vlr_gemv_w4 / vlr_gemv_w4_lora, 1 <= M <= 64 rows in one pass over the packed
// words.  Bit for bit the 16-row entry point on rows [0, 16), [16, 32), ... (gemv_w4_tile).  Workspace: the same split count times
// min(M, 64) rows; the adapter form takes vlr_gemv_wide_lora_workspace_bytes / vlr_gemv_wide_lora_u_bytes, which cover both split counts.
extern "C" long vlr_gemv_wide_w4_workspace_bytes(int M, int N, int K) {
    if (M < 1 || N < 1 || K < 8) return 0;
    return (long)gemv_splits(N, K, GW_COLS) * (M > 64 ? 64 : M) * N * 4;
}
extern "C" int vlr_gemv_wide_w4(int mode, const void* X, int ldx, const void* qweight, const void* qzeros, const void* scales,
                                int group_size, void* Y, int ldy, const void* bias, const void* residual, int ldr, const int* pos,
                                const float* cos_t, const float* sin_t, int rope_cols, int head_dim, int max_pos, int M, int N, int K,
                                void* workspace, vlr_stream_t st) {
    return gemv_w4_rows("vlr_gemv_wide_w4", 64, mode, X, ldx, qweight, qzeros, scales, group_size, Y, ldy, bias, residual, ldr, pos, cos_t,
                        sin_t, rope_cols, head_dim, max_pos, M, N, K, workspace, st);
}
extern "C" int vlr_gemv_wide_w4_lora(int mode, const void* X, int ldx, const void* qweight, const void* qzeros, const void* scales,
                                     int group_size, void* Y, int ldy, const void* bias, const void* residual, int ldr, const int* pos,
                                     const float* cos_t, const float* sin_t, int rope_cols, int head_dim, int max_pos, int M, int N, int K,
                                     void* workspace, const void* A, const void* B, int r, int targets, const int* outs, float scale,
                                     void* u, vlr_stream_t st) {
    if (!A && !B)
        return vlr_gemv_wide_w4(mode, X, ldx, qweight, qzeros, scales, group_size, Y, ldy, bias, residual, ldr, pos, cos_t, sin_t, rope_cols,
                                head_dim, max_pos, M, N, K, workspace, st);
    return gemv_w4_lora_rows("vlr_gemv_wide_w4_lora", 64, mode, X, ldx, qweight, qzeros, scales, group_size, Y, ldy, bias, residual, ldr,
                             pos, cos_t, sin_t, rope_cols, head_dim, max_pos, M, N, K, workspace, A, B, r, targets, outs, scale, u, st);
}

extern "C" int vlr_kv_cache_write(const void* k, const void* v, int ld, void* k_cache, void* v_cache, int batch, int S, int kv_heads,
                                  int head_dim, int cap, int slot0, vlr_stream_t st) {
    VLR_REQUIRE(k && v && k_cache && v_cache, "vlr_kv_cache_write: null argument");
    VLR_REQUIRE(batch >= 1 && S >= 1 && kv_heads >= 1 && head_dim >= 8 && head_dim % 8 == 0 && ld % 8 == 0 && ld >= kv_heads * head_dim,
                "vlr_kv_cache_write: bad shape (batch %d, S %d, kv_heads %d, head_dim %d, ld %d)", batch, S, kv_heads, head_dim, ld);
    VLR_REQUIRE(slot0 >= 0 && slot0 + S <= cap, "vlr_kv_cache_write: columns %d .. %d outside the cache capacity %d", slot0, slot0 + S - 1, cap);
    VLR_REQUIRE((((uintptr_t)k | (uintptr_t)v | (uintptr_t)k_cache | (uintptr_t)v_cache) & 15) == 0,
                "vlr_kv_cache_write: pointers must be 16-byte aligned");
    const long per = (long)batch * S * kv_heads * (head_dim / 8);
    hipLaunchKernelGGL(kv_cache_write_kernel, dim3((unsigned)((2 * per + 255) / 256)), dim3(256), 0, st, (const bf16_t*)k,
                       (const bf16_t*)v, ld, (bf16_t*)k_cache, (bf16_t*)v_cache, S, kv_heads, head_dim, cap, slot0, per);
    return vlr_check_launch("vlr_kv_cache_write");
}

extern "C" long vlr_attn_decode_workspace_bytes(int batch, int heads, int cap) {
    if (batch < 1 || heads < 1 || cap < 1) return 0;
    return (long)batch * heads * ((cap + AD_CMIN - 1) / AD_CMIN) * AD_REC * 4;
}

extern "C" int vlr_attn_decode_gqa(const void* q, int ldq, const void* k_cache, const void* v_cache, const int* key_mask, void* o, int ldo,
                                   void* workspace, int batch, int heads, int kv_heads, int head_dim, int cap, int len, float scale,
                                   vlr_stream_t st) {
    VLR_REQUIRE(q && k_cache && v_cache && key_mask && o && workspace, "vlr_attn_decode_gqa: null argument");
    VLR_REQUIRE(head_dim == AD_HD, "vlr_attn_decode_gqa: head_dim %d unsupported (the decode kernel takes head_dim 128)", head_dim);
    VLR_REQUIRE(batch >= 1 && kv_heads >= 1 && heads % kv_heads == 0, "vlr_attn_decode_gqa: heads %d is not a multiple of kv_heads %d",
                heads, kv_heads);
    const int G = heads / kv_heads;
    VLR_REQUIRE(G == 1 || G == 2 || G == 4 || G == 8, "vlr_attn_decode_gqa: heads / kv_heads = %d (1, 2, 4 or 8 supported)", G);
    VLR_REQUIRE(len >= 1 && len <= cap, "vlr_attn_decode_gqa: len %d outside 1 .. cap %d", len, cap);
    VLR_REQUIRE(ldq % 8 == 0 && ldq >= heads * head_dim && ldo >= heads * head_dim, "vlr_attn_decode_gqa: ldq %d / ldo %d too small or ldq not a multiple of 8", ldq, ldo);
    const int C = attn_decode_chunk(batch, kv_heads, len), nchunks = (len + C - 1) / C;
    const float sl2 = scale * 1.4426950408889634f;
    const dim3 grid(nchunks, kv_heads, batch);
#define AD_LAUNCH(GG)                                                                                                               \
    hipLaunchKernelGGL(attn_decode_kernel<GG>, grid, dim3(256), 0, st, (const bf16_t*)q, ldq, (const bf16_t*)k_cache,             \
                       (const bf16_t*)v_cache, key_mask, (float*)workspace, kv_heads, cap, len, C, nchunks, sl2)
    switch (G) {
        case 1: AD_LAUNCH(1); break;
        case 2: AD_LAUNCH(2); break;
        case 4: AD_LAUNCH(4); break;
        default: AD_LAUNCH(8); break;
    }
#undef AD_LAUNCH
    hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(heads, batch), dim3(AD_HD), 0, st, (const float*)workspace, (bf16_t*)o, ldo, heads,
                       kv_heads, nchunks);
    return vlr_check_launch("vlr_attn_decode_gqa");
}

// ---- decode attention over a SHARED prompt (generate(num_return_sequences = n): the n samples of a prompt attend the same prompt keys).
// Key side of sample p * fanout + j: the prompt segment of prompt p (k, v [prompts][kv_heads][prompt_cap][128], left-padded, masked by
// prompt_mask) followed by the sample's own tail (k, v [prompts * fanout][kv_heads][tail_cap][128], every column below tail_len attended).
//
// attn_shared_prompt_kernel<KT>: grid (chunk, kv head, prompt), 256 threads, chunk C = 64 KT keys.  The workgroup owns all R = fanout * G
// query rows (row j * G + g = sample j, head g of the group) and walks them in tiles of 16; rows beyond R are zero queries and are never
// written.  What is read from HBM is read once per chunk, whatever R is:
//   K   wave w holds the B fragments of its KT key tiles (16 keys x 128 dims: four 16-byte loads per lane, as gemv_tile's W operand) in
//       registers across all row tiles.  Q . K^T: v_mfma_f32_16x16x32_bf16, A = the tile's 16 query rows (16-byte loads of q), fp32
//       scores in the log2 domain, masked keys (and keys >= prompt_len, which are never loaded) set to -inf, as attn_decode_kernel has it.
//   V   P . V contracts over the key, and V is [key][dim]: the MFMA's B fragment wants 8 consecutive KEYS of one dim per lane.  The chunk
//       is therefore transposed ONCE through LDS (vt [dim][key]: 16-byte global loads of two key rows, 4-byte LDS stores of one dim's
//       key pair), and each wave lifts the B fragments of its 32 output dims - all C keys - into registers, where they stay across the
//       row tiles.  Masked keys and keys >= prompt_len are stored as zeros and never loaded, so their content cannot reach the output.
//   P   is ROUNDED TO bf16 for the second MFMA (the one source of error attn_decode_kernel does not have: 2^-9 relative per probability);
//       the chunk's `sum` is taken over the rounded values, so the weights the output is normalised by are the weights that were applied.
// Every wave owns 32 output dims over all keys of the chunk: no cross-wave reduction of the accumulator.  A chunk whose keys are all
// masked writes (max = -inf, sum = 0) and returns.  Partials: the record format of attn_decode_kernel, [prompt][kv head][chunk][R].
template <int KT>
__global__ __launch_bounds__(256) void attn_shared_prompt_kernel(const bf16_t* __restrict__ q, int ldq, const bf16_t* __restrict__ kp,
                                                                 const bf16_t* __restrict__ vp, const int* __restrict__ mask,
                                                                 float* __restrict__ ws, int kvh, int G, int fanout, int cap, int len,
                                                                 int nchunks, float sl2) {
    constexpr int C = 64 * KT, VS = C + 8, SS = C + 4;       // VS: bf16 row stride of vt / pb (rows stay 16-byte aligned), SS: of sc
    __shared__ __attribute__((aligned(16))) bf16_t vt[AD_HD * VS];
    __shared__ __attribute__((aligned(16))) bf16_t pb[16 * VS];
    __shared__ float sc[16][SS];
    const int c = blockIdx.x, hk = blockIdx.y, p = blockIdx.z;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int j0 = c * C, R = fanout * G;
    const bf16_t* kbase = kp + ((size_t)p * kvh + hk) * cap * AD_HD;
    const bf16_t* vbase = vp + ((size_t)p * kvh + hk) * cap * AD_HD;
    const int* km = mask + (size_t)p * cap;
    float* rec = ws + (((size_t)p * kvh + hk) * nchunks + c) * R * AD_REC;
    bool mine = false;
    for (int i = threadIdx.x; i < C; i += 256) mine |= j0 + i < len && km[j0 + i] != 0;
    if (!__syncthreads_or(mine)) {
        for (int rr = threadIdx.x; rr < R; rr += 256) { rec[(size_t)rr * AD_REC] = -INFINITY; rec[(size_t)rr * AD_REC + 1] = 0.f; }
        return;
    }
    // ---- V chunk -> vt [dim][key].  64 consecutive work items = 16 key pairs x 4 dim groups of 8: the 4-byte stores of a wave then
    // fall on 32 banks, two lanes each
    uint32_t* vt32 = reinterpret_cast<uint32_t*>(vt);
    for (int idx = threadIdx.x; idx < C * 8; idx += 256) {
        const int blk = idx >> 6, l = idx & 63;
        const int kpi = (blk >> 2) * 16 + (l >> 2), dg = (blk & 3) * 4 + (l & 3);
        const int ja = j0 + 2 * kpi, jb = ja + 1;
        const bool oka = ja < len && km[ja] != 0, okb = jb < len && km[jb] != 0;
        const u32x4 z{0u, 0u, 0u, 0u};
        const u32x4 a = oka ? *reinterpret_cast<const u32x4*>(vbase + (size_t)ja * AD_HD + dg * 8) : z;
        const u32x4 b = okb ? *reinterpret_cast<const u32x4*>(vbase + (size_t)jb * AD_HD + dg * 8) : z;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            vt32[(dg * 8 + 2 * e) * (VS / 2) + kpi] = (a[e] & 0xffffu) | (b[e] << 16);
            vt32[(dg * 8 + 2 * e + 1) * (VS / 2) + kpi] = (a[e] >> 16) | (b[e] & 0xffff0000u);
        }
    }
    // ---- K fragments of this wave's key tiles: lane (r, g) holds B[k = 8 g + j][n = r] = K[key 16 tile + r][dim 32 u + 8 g + j]
    const bf16x8 zero = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
    bf16x8 kf[KT][4];
    bool kvalid[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        const int j = j0 + (wv * KT + t) * 16 + r;
        const bool inr = j < len;
        kvalid[t] = inr && km[j] != 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) kf[t][u] = inr ? load8(kbase + (size_t)j * AD_HD + u * 32 + g * 8) : zero;
    }
    __syncthreads();
    // V fragments: B[k = 8 g + j][n = r] = V[key 32 ks + 8 g + j][dim 32 wv + 16 nt + r]
    bf16x8 vf[C / 32][2];
#pragma unroll
    for (int ks = 0; ks < C / 32; ++ks)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) vf[ks][nt] = load8(vt + (32 * wv + 16 * nt + r) * VS + ks * 32 + 8 * g);
    for (int t0 = 0; t0 < R; t0 += 16) {
        // ---- scores of 16 query rows: A[m = r][k = 8 g + j] = q[row t0 + r][dim 32 u + 8 g + j]; D[m = 4 g + i][n = r]
        const int rr = t0 + r;
        const bool qok = rr < R;
        const bf16_t* qrow = q + ((size_t)p * fanout + (qok ? rr / G : 0)) * ldq + (size_t)(hk * G + (qok ? rr % G : 0)) * AD_HD;
        bf16x8 qa[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) qa[u] = qok ? load8(qrow + u * 32 + g * 8) : zero;
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            f32x4 s{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int u = 0; u < 4; ++u) s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[u], kf[t][u], s, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) sc[4 * g + i][(wv * KT + t) * 16 + r] = kvalid[t] ? s[i] * sl2 : -INFINITY;
        }
        __syncthreads();      // also: every wave has left the previous tile's P . V, pb may be rewritten
        // ---- chunk softmax statistics: wave wv owns rows 4 wv .. 4 wv + 3; P -> bf16
        for (int rw = 4 * wv; rw < 4 * wv + 4; ++rw) {
            float x[KT], mx = -INFINITY;
#pragma unroll
            for (int e = 0; e < KT; ++e) { x[e] = sc[rw][lane + 64 * e]; mx = fmaxf(mx, x[e]); }
            mx = wave_max(mx);
            float l = 0.f;
#pragma unroll
            for (int e = 0; e < KT; ++e) {
                const bf16_t pr = f32_to_bf16(mx == -INFINITY ? 0.f : exp2f(x[e] - mx));
                pb[rw * VS + lane + 64 * e] = pr;
                l += bf16_to_f32(pr);
            }
            l = wave_sum(l);
            if (lane == 0 && t0 + rw < R) { rec[(size_t)(t0 + rw) * AD_REC] = mx; rec[(size_t)(t0 + rw) * AD_REC + 1] = l; }
        }
        __syncthreads();
        // ---- P . V: A[m = r][k = 8 g + j] = P[row r][key 32 ks + 8 g + j]; D[m = 4 g + i][n = r] = O[row 4 g + i][dim 32 wv + 16 nt + r]
        f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < C / 32; ++ks) {
            const bf16x8 pa = load8(pb + r * VS + ks * 32 + 8 * g);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) o[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, vf[ks][nt], o[nt], 0, 0, 0);
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (t0 + 4 * g + i < R) rec[(size_t)(t0 + 4 * g + i) * AD_REC + 4 + 32 * wv + 16 * nt + r] = o[nt][i];
    }
}

// grid (heads, prompts * fanout), 128 threads = one per feature: the prompt's chunks in order, then the sample's tail chunks in order
__global__ __launch_bounds__(128) void attn_shared_combine_kernel(const float* __restrict__ wsp, const float* __restrict__ wst,
                                                                  bf16_t* __restrict__ o, int ldo, int heads, int kvh, int fanout, int ncp,
                                                                  int nct) {
    const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
    const int G = heads / kvh, hk = h / G, g = h % G, p = b / fanout, R = fanout * G, rr = (b % fanout) * G + g;
    const float* pbase = wsp + ((size_t)p * kvh + hk) * ncp * R * AD_REC + (size_t)rr * AD_REC;
    const float* tbase = wst + ((size_t)b * kvh + hk) * nct * G * AD_REC + (size_t)g * AD_REC;
    const size_t ps = (size_t)R * AD_REC, ts = (size_t)G * AD_REC;
    float mx = -INFINITY;
    for (int c = 0; c < ncp; ++c) mx = fmaxf(mx, pbase[c * ps]);
    for (int c = 0; c < nct; ++c) mx = fmaxf(mx, tbase[c * ts]);
    float l = 0.f, acc = 0.f;
    if (mx != -INFINITY)
        for (int c = 0; c < ncp + nct; ++c) {
            const float* rc = c < ncp ? pbase + c * ps : tbase + (c - ncp) * ts;
            const float m = rc[0];
            if (m == -INFINITY) continue;
            const float w = exp2f(m - mx);
            l += w * rc[1];
            acc += w * rc[4 + d];
        }
    o[(size_t)b * ldo + (size_t)h * AD_HD + d] = f32_to_bf16(l > 0.f ? acc / l : 0.f);
}

// prompt chunk: 128 keys, 64 while that leaves the chip short of workgroups
static int attn_shared_chunk(int prompts, int kvh, int len) { return (long)prompts * kvh * ((len + 127) / 128) < AD_TARGET_WGS ? 64 : 128; }
static long attn_shared_prompt_floats(int prompts, int fanout, int heads, int prompt_cap) {
    return (long)prompts * fanout * heads * ((prompt_cap + 63) / 64) * AD_REC;
}

extern "C" long vlr_attn_decode_shared_workspace_bytes(int prompts, int fanout, int heads, int prompt_cap, int tail_cap) {
    if (prompts < 1 || fanout < 1 || heads < 1 || prompt_cap < 1 || tail_cap < 1) return 0;
    return attn_shared_prompt_floats(prompts, fanout, heads, prompt_cap) * 4 + vlr_attn_decode_workspace_bytes(prompts * fanout, heads, tail_cap);
}

extern "C" int vlr_attn_decode_shared(const void* q, int ldq, const vlr_kv_shared* kv, void* o, int ldo, void* workspace, int heads,
                                      int kv_heads, int head_dim, float scale, vlr_stream_t st) {
    VLR_REQUIRE(q && kv && o && workspace, "vlr_attn_decode_shared: null argument");
    VLR_REQUIRE(kv->k_prompt && kv->v_prompt && kv->prompt_mask && kv->k_tail && kv->v_tail, "vlr_attn_decode_shared: null cache pointer");
    VLR_REQUIRE(head_dim == AD_HD, "vlr_attn_decode_shared: head_dim %d unsupported (the decode kernels take head_dim 128)", head_dim);
    VLR_REQUIRE(kv_heads >= 1 && heads >= 1 && heads % kv_heads == 0, "vlr_attn_decode_shared: heads %d is not a multiple of kv_heads %d",
                heads, kv_heads);
    const int G = heads / kv_heads;
    VLR_REQUIRE(G == 1 || G == 2 || G == 4 || G == 8, "vlr_attn_decode_shared: heads / kv_heads = %d (1, 2, 4 or 8 supported)", G);
    VLR_REQUIRE(kv->prompts >= 1, "vlr_attn_decode_shared: prompts %d", kv->prompts);
    VLR_REQUIRE(kv->fanout >= 1, "vlr_attn_decode_shared: fanout %d must be at least 1", kv->fanout);
    VLR_REQUIRE(kv->prompt_len >= 1 && kv->prompt_len <= kv->prompt_cap, "vlr_attn_decode_shared: prompt_len %d outside 1 .. prompt_cap %d",
                kv->prompt_len, kv->prompt_cap);
    VLR_REQUIRE(kv->tail_len >= 1 && kv->tail_len <= kv->tail_cap, "vlr_attn_decode_shared: tail_len %d outside 1 .. tail_cap %d",
                kv->tail_len, kv->tail_cap);
    VLR_REQUIRE(ldq % 8 == 0 && ldq >= heads * head_dim && ldo >= heads * head_dim && ((uintptr_t)q & 15) == 0,
                "vlr_attn_decode_shared: ldq %d / ldo %d too small, ldq not a multiple of 8 or q not 16-byte aligned", ldq, ldo);
    VLR_REQUIRE((((uintptr_t)kv->k_prompt | (uintptr_t)kv->v_prompt | (uintptr_t)kv->k_tail | (uintptr_t)kv->v_tail) & 15) == 0,
                "vlr_attn_decode_shared: cache pointers must be 16-byte aligned");
    const int P = kv->prompts, n = kv->fanout, B = P * n;
    const float sl2 = scale * 1.4426950408889634f;
    float* wsp = (float*)workspace;
    float* wst = wsp + attn_shared_prompt_floats(P, n, heads, kv->prompt_cap);
    const int Cp = attn_shared_chunk(P, kv_heads, kv->prompt_len), ncp = (kv->prompt_len + Cp - 1) / Cp;
    const dim3 gp(ncp, kv_heads, P);
    if (Cp == 64)
        hipLaunchKernelGGL(attn_shared_prompt_kernel<1>, gp, dim3(256), 0, st, (const bf16_t*)q, ldq, (const bf16_t*)kv->k_prompt,
                           (const bf16_t*)kv->v_prompt, kv->prompt_mask, wsp, kv_heads, G, n, kv->prompt_cap, kv->prompt_len, ncp, sl2);
    else
        hipLaunchKernelGGL(attn_shared_prompt_kernel<2>, gp, dim3(256), 0, st, (const bf16_t*)q, ldq, (const bf16_t*)kv->k_prompt,
                           (const bf16_t*)kv->v_prompt, kv->prompt_mask, wsp, kv_heads, G, n, kv->prompt_cap, kv->prompt_len, ncp, sl2);
    // the samples' own tails: the grouped kernel with the tail as the cache and no mask
    const int Ct = attn_decode_chunk(B, kv_heads, kv->tail_len), nct = (kv->tail_len + Ct - 1) / Ct;
    const dim3 gt(nct, kv_heads, B);
#define AD_LAUNCH(GG)                                                                                                               \
    hipLaunchKernelGGL(attn_decode_kernel<GG>, gt, dim3(256), 0, st, (const bf16_t*)q, ldq, (const bf16_t*)kv->k_tail,            \
                       (const bf16_t*)kv->v_tail, (const int*)nullptr, wst, kv_heads, kv->tail_cap, kv->tail_len, Ct, nct, sl2)
    switch (G) {
        case 1: AD_LAUNCH(1); break;
        case 2: AD_LAUNCH(2); break;
        case 4: AD_LAUNCH(4); break;
        default: AD_LAUNCH(8); break;
    }
#undef AD_LAUNCH
    hipLaunchKernelGGL(attn_shared_combine_kernel, dim3(heads, B), dim3(AD_HD), 0, st, (const float*)wsp, (const float*)wst, (bf16_t*)o, ldo,
                       heads, kv_heads, n, ncp, nct);
    return vlr_check_launch("vlr_attn_decode_shared");
}
