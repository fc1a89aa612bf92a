// GPTQ int4 ("v1" checkpoint format, AutoGPTQ) - the one definition every kernel that reads packed weights shares (include/vlr.h
// "GPTQ int4 base weights").  A linear y = x W^T, W [N][K], group size g:
//   qweight int32 [K/8][N]   nibble j (bits 4j .. 4j+3) of qweight[k8][n] = q[8 k8 + j][n], 0 .. 15
//   qzeros  int32 [K/g][N/8] nibble j of qzeros[G][n8] = STORED zero of column 8 n8 + j; the zero used is stored + 1 (stored 15 -> 16)
//   scales  fp16  [K/g][N]
//   W[n][k] = bf16_rne(float(scales[k/g][n]) * float(q[k][n] - zero[k/g][n]))
// |q - zero| <= 16 has 5 significant bits and an fp16 scale 11: the fp32 product is exact, so the bf16 rounding is the only one.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;

// the zero (stored + 1) of column n from the qzeros word that holds columns 8 (n / 8) .. 8 (n / 8) + 7
__device__ __forceinline__ int w4_zero(uint32_t zword, int n) { return (int)((zword >> (4 * (n & 7))) & 15u) + 1; }

// one qweight word = 8 consecutive k of one column -> 8 bf16 in k order (16 bytes: a row segment of W, or one lane's B fragment of
// v_mfma_f32_16x16x32_bf16)
__device__ __forceinline__ u32x4 w4_unpack(uint32_t q, float scale, int zero) {
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int lo = (int)((q >> (8 * i)) & 15u) - zero, hi = (int)((q >> (8 * i + 4)) & 15u) - zero;
        o[i] = pack_bf16((float)lo * scale, (float)hi * scale);
    }
    return o;
}
