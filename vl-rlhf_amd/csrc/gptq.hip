// GPTQ int4 base weights (q_lora): packed qweight / qzeros / scales -> the bf16 W [N][K] (K contiguous) every GEMM of the library reads.
// The format and the one dequantisation rule are in gptq.h.
//
//   gptq_dequant_kernel  HBM-bound: 0.5 byte + scales read and 2 bytes written per weight.  The source is N-contiguous and the
//                        destination K-contiguous, but the transpose needs no exchange between lanes: one int32 of qweight IS 8
//                        consecutive k of one column, i.e. one 16-byte row segment of W once it is unpacked.  A lane loads 16 bytes
//                        (4 columns x 8 k) and stores four 16-byte segments, one per column.  A wave is laid out 8 (k8) x 8 (4-column
//                        groups): its load touches 8 source rows x 128 contiguous bytes and each of its four stores 8 destination
//                        rows x 128 contiguous bytes - whole cache lines on both sides, nothing staged in LDS.  The group's scales
//                        (8 bytes) and zeros (one word) are read once per lane: g is a multiple of 8, so a lane's 8 k share a group.
#include "../../include/vlr.h"
#include "gptq.h"

constexpr int GQ_K8 = 16;      // qweight rows (8 k each) per workgroup: 128 k
constexpr int GQ_N4 = 16;      // 4-column groups per workgroup: 64 columns

__global__ __launch_bounds__(256) void gptq_dequant_kernel(const uint32_t* __restrict__ qweight, const uint32_t* __restrict__ qzeros,
                                                           const uint16_t* __restrict__ scales, bf16_t* __restrict__ W, int K, int N,
                                                           int gsz) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int k8 = blockIdx.y * GQ_K8 + (wv >> 1) * 8 + (lane & 7);
    const int n = (blockIdx.x * GQ_N4 + (wv & 1) * 8 + (lane >> 3)) * 4;
    if (k8 >= K / 8 || n >= N) return;                 // N % 8 == 0 and n % 4 == 0: a lane's 4 columns are all in or all out
    const int G = (k8 * 8) / gsz;
    const u32x4 q = *reinterpret_cast<const u32x4*>(qweight + (size_t)k8 * N + n);
    const f16x4 sc = __builtin_bit_cast(f16x4, *reinterpret_cast<const u32x2*>(scales + (size_t)G * N + n));
    const uint32_t zw = qzeros[(size_t)G * (N / 8) + n / 8];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        *reinterpret_cast<u32x4*>(W + (size_t)(n + j) * K + (size_t)k8 * 8) = w4_unpack(q[j], (float)sc[j], w4_zero(zw, n + j));
}

extern "C" int vlr_gptq_dequant_bf16(const void* qweight, const void* qzeros, const void* scales, void* W, int K, int N, int group_size,
                                     vlr_stream_t st) {
    VLR_REQUIRE(qweight && qzeros && scales && W, "vlr_gptq_dequant_bf16: null argument");
    VLR_REQUIRE(K >= 8 && K % 8 == 0 && N >= 8 && N % 8 == 0, "vlr_gptq_dequant_bf16: K %d and N %d must be positive multiples of 8", K, N);
    VLR_REQUIRE(group_size == K || (group_size >= 32 && group_size % 32 == 0 && K % group_size == 0),
                "vlr_gptq_dequant_bf16: group_size %d must be K (%d) or a multiple of 32 that divides it", group_size, K);
    VLR_REQUIRE((((uintptr_t)qweight | (uintptr_t)W) & 15) == 0 && ((uintptr_t)scales & 7) == 0 && ((uintptr_t)qzeros & 3) == 0,
                "vlr_gptq_dequant_bf16: qweight / W must be 16-byte, scales 8-byte, qzeros 4-byte aligned");
    const dim3 grid((N / 4 + GQ_N4 - 1) / GQ_N4, (K / 8 + GQ_K8 - 1) / GQ_K8);
    VLR_REQUIRE(grid.y <= 65535, "vlr_gptq_dequant_bf16: K %d too large", K);
    hipLaunchKernelGGL(gptq_dequant_kernel, grid, dim3(256), 0, st, (const uint32_t*)qweight, (const uint32_t*)qzeros,
                       (const uint16_t*)scales, (bf16_t*)W, K, N, group_size);
    return vlr_check_launch("vlr_gptq_dequant_bf16");
}
