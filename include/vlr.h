/* vlr.h - C ABI of libvlr_hip.so, the MI355X (gfx950) DPO-step library.
 *
 * Drop-in boundary.  The reference (TideDra/VL-RLHF) has no FFI: its hot path is Python that
 * bottoms out in torch/transformers/trl native code.  These entry points are what a binding for that path binds
 * instead; each cites the reference interface (file:line under /root/reference) whose arithmetic it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless said otherwise; "bf16" tensors are raw uint16 bit patterns;
 *   - row-major, leading dimensions (`ld*`) in ELEMENTS; no allocation inside: the caller passes workspaces;
 *   - every function enqueues on `stream` and returns immediately: 0 = ok, non-zero = error, message from
 *     vlr_last_error() (thread-local).  Argument errors map to Python ValueError in the host mirror;
 *   - thread-compatible, not thread-safe per stream; one process per GPU.
 */
#ifndef VLR_H
#define VLR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* vlr_stream_t; /* == hipStream_t */

const char* vlr_last_error(void);
int vlr_abi_version(void);
/* in-library kernel timing (HIP events on the launch stream): kernels 0 gemm NT, 1 gemm NN, 2 gemm TN, 3 attention fwd,
 * 4 attention bwd, 5 the 256x256 eight-phase GEMM kernel alone (the sub-launches of 0-2).  vlr_prof_collect fills out[k*3 + {0,1,2}] = {launches, total ms, algorithmic FLOPs}.
 * vlr_prof_enable(0) stops; (N >= 1) starts and brackets one launch in N, picked pseudo-randomly per kernel id - launches and FLOPs
 * stay exact, `total ms` is the sampled mean x launches (an event pair is two queue packets around the kernel: N = 1 perturbs the step). */
int vlr_prof_enable(int on);
int vlr_prof_collect(double* out_host, int n_kernels);

/* ---- GEMM (replaces torch.nn.functional.linear / its autograd on cuBLAS: every nn.Linear under
 *      LlavaForRL.forward, src/vlrlhf/models/Llava/__init__.py:178,191,232) --------------------------------------
 * layout 0 (NT): C[M,N] = A[M,K] . B[N,K]^T         forward   y = x W^T
 * layout 1 (NN): C[M,N] = A[M,K] . B[K,N]           dgrad     dx = dy W
 * layout 2 (TN): C[M,N] = A[K,M]^T . B[K,N]         wgrad     dW = dy^T x
 * epilogue: v = act(acc + bias[n]) + residual[m,n] (+ C[m,n] if accumulate); act 0 none, 1 quick_gelu, 2 gelu(erf).
 * C is bf16 (out_f32 = 0) or fp32. */
int vlr_gemm_bf16(int layout, const void* A, const void* B, void* C, const void* bias, const void* residual, int M,
                  int N, int K, int lda, int ldb, int ldc, int ldr, int act, int accumulate, int out_f32,
                  vlr_stream_t stream);
/* same with v = act(alpha * acc + bias) + ...  (peft LoRA merge W_eff = W + (lora_alpha / r) * B A; call site of the
 * adapters: /root/reference src/vlrlhf/utils/auto_load.py:559-571) */
int vlr_gemm_bf16_scaled(int layout, const void* A, const void* B, void* C, const void* bias, const void* residual, int M,
                         int N, int K, int lda, int ldb, int ldc, int ldr, int act, int accumulate, int out_f32,
                         float alpha, vlr_stream_t stream);
/* Two weight-gradient GEMMs of one decoder layer in one launch (layout 2 of vlr_gemm_bf16, both over the same K token rows):
 * C0 [M0][N0] = A0^T B0 and C1 [M1][N1] = A1^T B1 (A_i [K][lda_i], B_i [K][ldb_i], bf16; accumulate as in vlr_gemm_bf16).  The output tiles
 * of both problems form ONE persistent grid, so their tile counts add up before they are rounded to whole rounds of the CUs - the
 * dW of gate|up and of down_proj of LLaMA-7B are 6 + 3 rounds apart and 8 together.  Same arithmetic and results as two vlr_gemm_bf16
 * calls (which it falls back to when the shapes do not qualify).  Replaces two of the cuBLAS wgrad calls under autograd's backward of
 * transformers LlamaMLP (call site src/vlrlhf/models/Llava/__init__.py:232-243). */
int vlr_gemm_bf16_tn_pair(const void* A0, const void* B0, void* C0, int M0, int N0, int lda0, int ldb0, int ldc0, const void* A1,
                          const void* B1, void* C1, int M1, int N1, int lda1, int ldb1, int ldc1, int K, int accumulate,
                          vlr_stream_t stream);
/* fp32 residual stream (vlr_llama_cfg.resid_f32): C fp32 [M][ldc] = A . B (layout as above) + residual fp32 [M][ldr] (NULL: none);
 * in place (C == residual) is allowed.  Replaces the `hidden_states = residual + hidden_states` adds of transformers
 * LlamaDecoderLayer.forward (call site src/vlrlhf/models/Llava/__init__.py:232) without the bf16 rounding of the sum. */
int vlr_gemm_bf16_f32res(int layout, const void* A, const void* B, float* C, const float* residual, int M, int N, int K,
                         int lda, int ldb, int ldc, int ldr, vlr_stream_t stream);
/* Switches of the persistent (continuous-pipeline) GEMM launches, a sum of: 8 = the adapter-segment K tiles take the general staging
 * path, 16 = the two wave groups of a workgroup run their epilogues one after the other (the order before round 4; bit-identical
 * results), 32 = the shared-panel tile map (csrc/gemm_tilemap.h, round 5: the XCD blocks of a round are stacked into one super-block so
 * that the eight XCDs share panels through the Infinity Cache; same results, other order of the output tiles).  Production = 32.
 * -1 = back to the default (environment VLR_GEMM_SCHED, else 32).  The tile schedules 1-7 of ABI v5 (stream-K tail, XCD rotation, XCD
 * round barrier) measured slower or neutral and are rejected with VLR_ERR_ARG. */
int vlr_gemm_set_sched(int mode);
/* Diagnostics only: the tile timeline of the persistent GEMM launches.  With a non-NULL buffer of >= 256 KiB every later launch of the
 * 256x256 continuous-pipeline kernel leaves, for each workgroup b, words [b*256 + 4*i .. +3] = {tile id, and the 100 MHz clock after the
 * first K tile / after the K loop / after the epilogue's stores were issued} of its i-th tile, and [b*256 + 252 ..] = {tiles, start
 * clock, K tiles per tile}.  Recorded only by the library built with -DVLR_GEMM_TRACE (`build_hip.py --trace`,
 * tools/gemm_tile_trace.py); the production build returns VLR_ERR_ARG.  (NULL, 0) switches it off. */
int vlr_gemm_set_trace(void* buf, long bytes);
/* Optional fp32 scratch for split-K: problems with few output tiles and a long reduction (the LoRA adapter gradients;
 * the ragged last tile rows of the decoder GEMMs) are split along K into fp32 partials and reduced by a second kernel
 * that applies the epilogue.  Without it they run un-split.  The buffer is cut in 128 MiB slots (at most eight; below 256 MiB in
 * total: 64 MiB slots, which cover the split-K partials of the 7B shapes), one per
 * distinct stream that launches such a GEMM (policy pass, reference pass on a side stream, ...); further streams run un-split.
 * Registering again forgets the stream assignment.  (NULL, 0) unregisters. */
int vlr_gemm_set_splitk_workspace(void* workspace, long bytes);
/* Fused forward projections of the decoder layer (transformers LlamaMLP / LlamaAttention; call site
 * src/vlrlhf/models/Llava/__init__.py:232).  The elementwise op that follows the projection runs on the fp32 accumulators
 * in the GEMM epilogue - one rounding to bf16 instead of two and no extra pass over the tensor.
 *  vlr_gemm_swiglu  : gu [M][2I] = x [M][K] . wgu[2I][K]^T (gate | up), act [M][I] = silu(gate) * up; store_gu = 0 skips writing
 *                     gu where the fused kernel runs (no-grad passes; gu must still be a valid scratch buffer).
 *  vlr_gemm_qkv_rope: qkv [M][N] = x . wqkv[N][K]^T with rotate-half RoPE by pos[row] on the first rope_cols columns (the q and k
 *                     heads; head_dim 128 takes the fused path, other sizes the plain GEMM + vlr_rope). */
int vlr_gemm_swiglu(const void* x, const void* wgu, void* gu, void* act, int M, int I, int K, int ldx, int store_gu,
                    vlr_stream_t stream);
int vlr_gemm_qkv_rope(const void* x, const void* wqkv, void* qkv, const int* pos, const float* cos_t, const float* sin_t, int M,
                      int N, int rope_cols, int K, int ldx, int head_dim, int max_pos, vlr_stream_t stream);
/*  vlr_gemm_qkv_rope_bias: the same with a bias [N] on the projection (Qwen c_attn, QwenVL/modeling_qwen.py:104), NULL = none */
int vlr_gemm_qkv_rope_bias(const void* x, const void* wqkv, const void* bias, void* qkv, const int* pos, const float* cos_t,
                           const float* sin_t, int M, int N, int rope_cols, int K, int ldx, int head_dim, int max_pos, vlr_stream_t stream);
/*  vlr_gemm_swiglu_bwd: backward of the MLP's first half in one pass - d act = dy [M][H] . wdown [H][I] stays in the
 *                     accumulators and gu [M][2I] (gate | up of the forward) is replaced in place by d gate | d up.  dact_ws
 *                     [M][I] is scratch for the rows / shapes that take the plain GEMM + vlr_swiglu_bwd. */
int vlr_gemm_swiglu_bwd(const void* dy, const void* wdown, void* gu_inout, void* dact_ws, int M, int I, int H,
                        vlr_stream_t stream);
/*  vlr_gemm_swiglu_bwd_src: the same OUT OF PLACE through a source-row map (additive: vlr_abi_version() does not move) - gate | up of
 *                     row m are row src_rows[m] of gu_src [Mc][2I] (the kept rows of a row-compact forward; read only, rows may
 *                     repeat), [d gate | d up] go to row m of dgu_out [M][2I].  src_rows: M device int32 in [0, Mc), not checked by
 *                     the kernels.  dgu_out must not overlap gu_src (refused where the library can see it).  Peel, route and
 *                     arithmetic are vlr_gemm_swiglu_bwd's at M rows - its bits on gate | up expanded through src_rows; rows that
 *                     fall back take the plain GEMM + vlr_swiglu_bwd_src.  There is no addend form. */
int vlr_gemm_swiglu_bwd_src(const void* dy, const void* wdown, const void* gu_src, const int* src_rows, void* dgu_out, void* dact_ws,
                            int M, int I, int H, vlr_stream_t stream);
/* The forward NT products of a decoder layer with an M-SIDE ROW MAP on the A operand (additive: vlr_abi_version() does not move): logical
 * row m of x / a is row a_rows[m] of the buffer (M device int32, every entry a valid buffer row, not checked; rows may repeat and need not
 * ascend).  The map is read once per output tile and on the general staging path (K % 64 != 0, the next tile's first K tiles), never in
 * the steady-state K loop.  Same launches, kernels and K order as vlr_gemm_qkv_rope_bias / vlr_gemm_swiglu / vlr_gemm_bf16[_f32res] on a
 * gathered A: the same bits.  Only the persistent 256-tile kernels take a map: a shape they refuse is an ERROR here, not a fallback.
 * vlr_gemm_res_rows: y [M][N] (fp32 if f32, else bf16) = a W^T + res, NT, lda = ldb = K, ldc = ldr = N.  peel_rows > 0: the LAST
 * peel_rows logical rows run on the 128x128 split-K kernel, which takes a plain pointer: they must be the contiguous buffer rows
 * tail_row0 .. tail_row0 + peel_rows - 1 (not checked).  0: none. */
int vlr_gemm_qkv_rope_bias_rows(const void* x, const int* a_rows, const void* wqkv, const void* bias, void* qkv, const int* pos,
                                const float* cos_t, const float* sin_t, int M, int N, int rope_cols, int K, int ldx, int head_dim,
                                int max_pos, vlr_stream_t stream);
int vlr_gemm_swiglu_rows(const void* x, const int* a_rows, const void* wgu, void* gu, void* act, int M, int I, int K, int ldx, int store_gu,
                         vlr_stream_t stream);
int vlr_gemm_res_rows(int f32, const void* a, const int* a_rows, const void* W, void* y, const void* res, int M, int N, int K,
                      int peel_rows, int tail_row0, vlr_stream_t stream);
/* The two fused products with OUTPUT ROW MAPS (additive: vlr_abi_version() does not move): what the epilogue computed for logical row m
 * is stored at row c_rows[m] of the destination and, where c_twin[m] >= 0, at row c_twin[m] too - the same registers, one rounding.
 * c_rows, c_twin: M device int32 each, valid destination rows (c_twin: or -1), not checked; no two logical rows may name the same
 * destination row.  Destination rows that no entry names are not written.  pos, the bias and the rotation stay indexed by the logical
 * row.  a_rows: an A-side map as above, or NULL (x read in place).  Launches, kernels, K order and values are those of
 * vlr_gemm_qkv_rope_bias[_rows] / vlr_gemm_swiglu[_rows]: the result equals theirs followed by vlr_gather_rows, bit for bit.
 * vlr_gemm_swiglu_dst: act alone goes through the maps (act_dst [.][I]); gate | up (store_gu) are written on the M logical rows of gu.
 * Its mapped kernel exists with an A-side map only.
 * Shapes the fused persistent kernel does not take (head_dim != 128, widths off its tiles, K < 256, unaligned operands; for SwiGLU also
 * a_rows == NULL) fall back: the unmapped product into qkv_rows / act_rows [M rows], then vlr_gather_rows through dense_src [Md] (for
 * every destination row the logical row that holds its value) into the Md destination rows - the fallback needs these three and an
 * unmapped x, and reports an error without them.  The destination must not be x, gu or the fallback buffer. */
int vlr_gemm_qkv_rope_bias_dst(const void* x, const int* a_rows, const void* wqkv, const void* bias, void* qkv_dst, const int* c_rows,
                               const int* c_twin, void* qkv_rows, const int* dense_src, int Md, const int* pos, const float* cos_t,
                               const float* sin_t, int M, int N, int rope_cols, int K, int ldx, int head_dim, int max_pos,
                               vlr_stream_t stream);
int vlr_gemm_swiglu_dst(const void* x, const int* a_rows, const void* wgu, void* gu, void* act_dst, const int* c_rows, const int* c_twin,
                        void* act_rows, const int* dense_src, int Md, int M, int I, int K, int ldx, int store_gu, vlr_stream_t stream);
/* The same projections with the LoRA adapters of the group riding the K loop of the base GEMM (peft lora.Linear.forward,
 * result = base(x) + lora_B(lora_A(dropout(x))) * scaling; reference targets src/vlrlhf/models/Llava/__init__.py:273-286):
 * after the K tiles of x . W^T the kernel runs on into u . Bl^T, u [M][ldu] = scaling * dropout_t(x) A_t^T of the group's
 * targets side by side (r columns each, written by the caller's lora_A GEMMs), Bl = the lora_B rows of the group [N][r].  The
 * adapter term is block-diagonal: an output tile of target t multiplies only u_t.  One rounding, fused SwiGLU / RoPE / residual
 * epilogues as above; shapes / rows the persistent kernel does not take run base GEMM + one skinny GEMM per target.
 *  vlr_gemm_lora         : y [M][ldy] = x [M][K] . W[N][K]^T + u . Bl^T (+ residual [M][ldr])          (o_proj, down_proj)
 *  vlr_gemm_swiglu_lora  : gate | up with u = u_gate | u_up, Bl = [B_gate ; B_up] [2I][r]; gu is always stored
 *  vlr_gemm_qkv_rope_lora: q | k | v with u = u_q | u_k | u_v, Bl = [B_q ; B_k ; B_v]; q_cols + 2 * kv_cols = N.  kv_cols = 0: ONE
 *                          adapter over the whole fused projection (u [M][r], Bl [N][r]).  bias [N] (NULL = none) is added before
 *                          the rotation. */
/*  vlr_gemm_dropout_acc  : dx [M][in] += scaling / (1 - p) * mask .* (v [M][ldv] . A [r][in]) - the input-gradient term of one
 *                          target under lora_dropout; the mask is regenerated from (seed, row * in + col) as in vlr_dropout and the
 *                          product never reaches HBM (scratch [M][in] only for shapes the fused kernel does not take) */
/*  vlr_gemm_grouped     : `groups` (<= 8) equally shaped skinny GEMMs as ONE launch - group g computes C + g gC = alpha * (A + g gA) . (B + g gB)
 *                          (layout as vlr_gemm_bf16, strides in elements, bf16 out, optional += C) - the per-target lora_A / lora_B products of a
 *                          fused group (q, k, v / gate, up), split along K when that fills the chip.  mask_on 1 (NT) / 2 (TN): the activation
 *                          operand (A rows / B rows, dense [rows][mask_ld]) is multiplied by the keep mask of vlr_dropout(seed + g) while it is
 *                          staged - lora_dropout without a dropped copy of x; the caller folds 1 / (1 - p) into alpha. */
int vlr_gemm_grouped(int layout, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, int groups,
                     long gA, long gB, long gC, float alpha, int accumulate, int mask_on, uint64_t seed, float p_drop, int mask_ld,
                     vlr_stream_t stream);
int vlr_gemm_dropout_acc(const void* v, int ldv, const void* A, void* dx, void* scratch, int M, int in, int r, float p,
                         uint64_t seed, float scale, vlr_stream_t stream);
/*  vlr_gemm_dropout_acc_multi: the same for the n targets that share dx, in ONE pass over it: dx (+)= scaling / (1 - p) * sum_t mask_t .*
 *                          (v_t . A_t), v [M][ldv] = the n blocks of r columns side by side, A = the n stacked [r][in] matrices, mask_t of
 *                          vlr_dropout(seed + t); accumulate = 0 WRITES dx (the adapter term alone) */
int vlr_gemm_dropout_acc_multi(int n, const void* v, int ldv, const void* A, void* dx, int M, int in, int r, float p, uint64_t seed,
                               float scale, int accumulate, vlr_stream_t stream);
/*  ..._bits (ABI v5)     : the three calls above with the keep masks DRAWN BEFOREHAND by vlr_dropout_bits (packed, bit e of byte i =
 *                          element 8 i + e of the dense [rows][mask_ld] operand; the mask of group / target g starts at bits + g *
 *                          gstride bytes, seed + g as before): the forward, the dA and the dx kernels of a target all need the same mask
 *                          and the packed form lets the masked operand travel by LDS-DMA (gemm128p.hip masks the fragments it reads).
 *                          vlr_gemm_grouped_bits: mask_on 1 / 2 read the row-major masks, mask_on 3 (layout 2) the K-tile-blocked transposed
 *                          ones of vlr_dropout_bits2.  bits = NULL: hash in the kernel, exactly the calls above. */
int vlr_gemm_grouped_bits(int layout, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, int groups,
                          long gA, long gB, long gC, float alpha, int accumulate, int mask_on, uint64_t seed, float p_drop, int mask_ld,
                          const void* mask_bits, long mask_gstride, vlr_stream_t stream);
int vlr_gemm_dropout_acc_bits(const void* v, int ldv, const void* A, void* dx, void* scratch, int M, int in, int r, float p,
                              uint64_t seed, float scale, const void* bits, vlr_stream_t stream);
int vlr_gemm_dropout_acc_multi_bits(int n, const void* v, int ldv, const void* A, void* dx, int M, int in, int r, float p, uint64_t seed,
                                    float scale, int accumulate, const void* bits, long bits_gstride, vlr_stream_t stream);
/*  ..._rows (ABI v7)     : the adapter restricted to a ROW SET (InternLM-XComposer2's PLoRA acts on the image rows only, reference
 *                          models/InternLMXC2/build_mlp.py:194-202).  rowmask [M] bytes, 1 = the row takes part.
 *                          vlr_gemm_grouped_bits_rows (layouts 0 / 1, accumulate 0): 128-row output tiles without a marked row are not
 *                          computed - the caller zeroes the unmarked rows afterwards (vlr_rows_mask), which it does anyway.
 *                          vlr_gemm_dropout_acc_multi_rows: the caller guarantees zero v rows on the unmarked rows; with accumulate = 1
 *                          every 64-row slab without a marked row is skipped (dx += 0).  rowmask = NULL: the calls above. */
int vlr_gemm_grouped_bits_rows(int layout, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, int groups,
                               long gA, long gB, long gC, float alpha, int accumulate, int mask_on, uint64_t seed, float p_drop,
                               int mask_ld, const void* mask_bits, long mask_gstride, const unsigned char* rowmask, vlr_stream_t stream);
/*  vlr_rows_tile_list    : out[0] = n, out[1 .. n] = the 64-row tiles of [0, M) with a marked row, ascending (out: M / 64 + 2 ints).
 *  vlr_gemm_grouped_bits_ktiles (layout 2, C = A^T B over K = token rows, K % 64 == 0): contracts only over the listed K tiles - the
 *                          caller guarantees that every other row contributes zero (PLoRA's dB = dy^T u, dA = v^T drop(x)).  The list
 *                          is read on the device; split-K slices cut the LIST, so the summation order differs from the dense call. */
int vlr_rows_tile_list(const unsigned char* rowmask, int M, int* out, vlr_stream_t stream);
/* (ABI v8) vlr_rows_tile_flags: flags[t] = 1 when NO row of the tile_rows-row tile t of [0, M) is marked (ceil(M / tile_rows) bytes).
 * vlr_gemm_seg_rowskip(tile_flags, keep): the NEXT adapter-segment GEMM call of this thread (vlr_gemm_lora[_f32res] / vlr_gemm_swiglu_lora /
 * vlr_gemm_qkv_rope_lora) may run the 256-row tiles whose flag is set over only the first `keep` (multiple of 64; 0 = none) K elements of
 * every sub-target's r-wide block of the segment - the caller guarantees that the REST of u is zero on the rows of those tiles, so the
 * result is bit-identical to the full segment.  InternLM-XComposer2: the [u_lora | u_plora] segment of the two-adapter passes with keep =
 * r_lora (PLoRA acts on the image rows only: reference models/InternLMXC2/build_mlp.py:194-202), and PLoRA alone with keep = 0.
 * tile_flags = NULL clears a pending setting. */
int vlr_rows_tile_flags(const unsigned char* rowmask, int M, int tile_rows, unsigned char* flags, vlr_stream_t stream);
int vlr_gemm_seg_rowskip(const unsigned char* tile_flags, int keep);
int vlr_gemm_grouped_bits_ktiles(int layout, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, int groups,
                                 long gA, long gB, long gC, float alpha, int accumulate, int mask_on, uint64_t seed, float p_drop,
                                 int mask_ld, const void* mask_bits, long mask_gstride, const int* ktlist, vlr_stream_t stream);
int vlr_gemm_dropout_acc_multi_rows(int n, const void* v, int ldv, const void* A, void* dx, int M, int in, int r, float p, uint64_t seed,
                                    float scale, int accumulate, const void* bits, long bits_gstride, const unsigned char* rowmask,
                                    vlr_stream_t stream);
/* (ABI v9) The row-slab adapter products, streamed (csrc/lora_rows.hip): a workgroup owns 64 token rows and reads its rows of the
 * activation ONCE at HBM rate straight into MFMA fragments, the small matrix travels through an LDS ring; no split-K partials, no
 * reduction launch, bit-reproducible.  r in {64, 128, 256}; in / outs multiples of 64; rows 16-byte aligned.
 *  vlr_lora_rows_u: u [M][t * ustride .. + r] = alpha * (keep_t . x [M][in]) . A_t [r][in]^T for the n <= 4 targets that share x (A = the
 *                   stacked A_t; peft lora.Linear.forward: lora_A(dropout(x)) * scaling, reference utils/auto_load.py:559-571).  bits = the
 *                   packed keep masks of vlr_dropout_bits (target t at bits + t * bits_gstride; x dense, ldx == in) or NULL (no dropout).
 *  vlr_lora_rows_v: v [M][t * r .. + r] = dy [M][ofs_t .. + outs[t]] . B_t [outs[t]][r], B = the stacked B_t, ofs_t = outs[0] + .. + outs[t-1]
 *                   (outs: HOST array) - the input of the dA / dx terms of the backward.
 *  rowmask [M] bytes or NULL: a row-restricted adapter (InternLM-XComposer2's PLoRA, reference models/InternLMXC2/build_mlp.py:194-202) -
 *                   unmarked rows come out ZERO, 64-row slabs without a marked row are not read. */
int vlr_lora_rows_u(int n, const void* x, int ldx, const void* A, void* u, int ldu, int ustride, int M, int in, int r, float alpha,
                    const void* bits, long bits_gstride, const unsigned char* rowmask, vlr_stream_t stream);
int vlr_lora_rows_v(int n, const void* dy, int lddy, const int* outs, const void* B, void* v, int ldv, int M, int r,
                    const unsigned char* rowmask, vlr_stream_t stream);
/*  vlr_gemm_swiglu_bwd_add: vlr_gemm_swiglu_bwd with an addend on d act before the SwiGLU backward (d act = dy . wdown + dact_add, bf16
 *                          [M][I]; may be the dact_ws buffer) - the LoRA adapter term of down_proj */
int vlr_gemm_swiglu_bwd_add(const void* dy, const void* wdown, void* gu_inout, void* dact_ws, const void* dact_add, int M, int I, int H,
                            vlr_stream_t stream);
int vlr_gemm_lora(const void* x, int ldx, const void* W, void* y, int ldy, const void* residual, int ldr, int M, int N, int K,
                  const void* u, int ldu, const void* Bl, int r, vlr_stream_t stream);
/*  vlr_gemm_lora_f32res  : the same on the fp32 residual stream - y fp32 [M][ldy] = x W^T + u Bl^T + residual fp32 [M][ldr] */
int vlr_gemm_lora_f32res(const void* x, int ldx, const void* W, float* y, int ldy, const float* residual, int ldr, int M, int N, int K,
                         const void* u, int ldu, const void* Bl, int r, vlr_stream_t stream);
int vlr_gemm_swiglu_lora(const void* x, const void* wgu, void* gu, void* act, int M, int I, int K, int ldx, const void* u, int ldu,
                         const void* Bl, int r, vlr_stream_t stream);
int vlr_gemm_qkv_rope_lora(const void* x, const void* wqkv, const void* bias, void* qkv, const int* pos, const float* cos_t,
                           const float* sin_t, int M, int N, int rope_cols, int K, int ldx, int head_dim, int max_pos, const void* u,
                           int ldu, const void* Bl, int r, int q_cols, int kv_cols, vlr_stream_t stream);

/* ---- normalisation / activations (transformers LlamaRMSNorm, CLIP LayerNorm, SwiGLU, GELU; call sites
 *      Llava/__init__.py:178-191,232) ------------------------------------------------------------------------- */
int vlr_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int M, int H, float eps, vlr_stream_t stream);
/* x fp32 [M][H] (fp32 residual stream); y bf16 */
int vlr_rmsnorm_fwd_f32(const float* x, const void* w, void* y, float* rstd, int M, int H, float eps, vlr_stream_t stream);
int vlr_rmsnorm_bwd_workspace_bytes(int H);
int vlr_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, const void* dres, void* dx,
                    void* dw, int dw_accumulate, void* workspace, int M, int H, vlr_stream_t stream);
/* the same with the forward input x in fp32; dy / dres / dx (the gradient stream) are bf16 */
int vlr_rmsnorm_bwd_f32(const void* dy, const float* x, const void* w, const float* rstd, const void* dres, void* dx,
                        void* dw, int dw_accumulate, void* workspace, int M, int H, vlr_stream_t stream);
/* The two above with x and rstd read through a SOURCE-ROW MAP (additive: vlr_abi_version() does not move): x [Mc][H] and rstd [Mc] hold
 * the kept rows of a row-compact forward, and dense row m of the backward is row src_rows[m] of them.  src_rows: M device int32, every
 * entry in [0, Mc) - the kernels do not check it; rows may repeat.  dy, dres, dx are dense [M][H]; dx must not overlap x.  The row walk,
 * the dw partials and their reduction are the unmapped call's: the result is that call's on x / rstd expanded through src_rows, bit
 * for bit. */
int vlr_rmsnorm_bwd_src(const void* dy, const void* x, const void* w, const float* rstd, const void* dres, void* dx, void* dw,
                        int dw_accumulate, void* workspace, const int* src_rows, int M, int H, vlr_stream_t stream);
int vlr_rmsnorm_bwd_f32_src(const void* dy, const float* x, const void* w, const float* rstd, const void* dres, void* dx, void* dw,
                            int dw_accumulate, void* workspace, const int* src_rows, int M, int H, vlr_stream_t stream);
/* RMSNorm forward of the kept rows of a row-compact pass, written DENSELY (additive): x [Mc][H] and rstd [Mc] hold the kept rows; row j of
 * the result goes to row compact_rows[j] of y and, where twin[j] >= 0 (a shared row), to row twin[j] as well - the maps vlr_fold_rows
 * reads (vlr_row_maps).  Rows of y that no kept row maps to are not written.  The values are vlr_rmsnorm_fwd's, bit for bit. */
int vlr_rmsnorm_fwd_scatter(const void* x, const void* w, void* y, float* rstd, const int* compact_rows, const int* twin, int Mc, int H,
                            float eps, vlr_stream_t stream);
int vlr_rmsnorm_fwd_f32_scatter(const float* x, const void* w, void* y, float* rstd, const int* compact_rows, const int* twin, int Mc, int H,
                                float eps, vlr_stream_t stream);
int vlr_layernorm_fwd(const void* x, const void* w, const void* b, void* y, int M, int D, float eps, vlr_stream_t stream);
/* backward of y = LayerNorm(x) * w + b (Qwen-VL resampler: ln_q / ln_kv / ln_post, QwenVL/visual.py:122-123,391): mean and rstd are
 * recomputed from x; dx may be NULL, dw / db (bf16 [D], `accumulate`: +=) may be NULL; workspace = vlr_layernorm_bwd_workspace_bytes(D) */
int vlr_layernorm_bwd_workspace_bytes(int D);
int vlr_layernorm_bwd(const void* dy, const void* x, const void* w, float eps, void* dx, void* dw, void* db, int accumulate,
                      void* workspace, int M, int D, vlr_stream_t stream);
int vlr_vit_embed_ln(const void* patch_embeds, const void* cls, const void* pos, const void* w, const void* b, void* y,
                     int n_img, int T, int D, float eps, vlr_stream_t stream);
/* backward of vlr_vit_embed_ln: dy [n_img*T][D] is the gradient of its output.  Recomputes cat(cls, patch_embeds) + pos and the
 * LayerNorm statistics; writes d_patch_embeds [n_img*(T-1)][D] (overwritten) and d_cls [D], d_pos [T][D], d_w, d_b [D] (bf16;
 * `accumulate`: +=).  The sums over images and rows run in a fixed order (no atomics); workspace = vlr_layernorm_bwd_workspace_bytes(D). */
int vlr_vit_embed_ln_bwd(const void* dy, const void* patch_embeds, const void* cls, const void* pos, const void* w,
                         void* d_patch_embeds, void* d_cls, void* d_pos, void* d_w, void* d_b, int accumulate, void* workspace,
                         int n_img, int T, int D, float eps, vlr_stream_t stream);
/* vlr_layernorm_bwd with the gradient of the residual branch around the norm: dx = dres + (LayerNorm backward), rounded once; dx may
 * be dres.  dw and db are required. */
int vlr_layernorm_bwd_res(const void* dy, const void* x, const void* w, float eps, const void* dres, void* dx, void* dw, void* db,
                          int accumulate, void* workspace, int M, int D, vlr_stream_t stream);
int vlr_im2col(const float* pixel_values, void* patches, int n_img, int image_size, int patch, int Kp, vlr_stream_t stream);
int vlr_rope_table(float* cos_t, float* sin_t, int max_pos, int head_dim, float theta, vlr_stream_t stream);
int vlr_rope(void* qkv, const int* pos, const float* cos_t, const float* sin_t, int M, int H, int head_dim, int ld,
             int max_pos, int backward, vlr_stream_t stream);
/* same on the first n_heads heads of every row (q heads followed by the k heads; grouped-query layouts have fewer k heads) */
int vlr_rope_heads(void* qkv, const int* pos, const float* cos_t, const float* sin_t, int M, int n_heads, int head_dim, int ld,
                   int max_pos, int backward, vlr_stream_t stream);
int vlr_swiglu_fwd(const void* gate_up, void* act, int M, int I, vlr_stream_t stream);
int vlr_swiglu_bwd(void* gate_up_inout, const void* dact, int M, int I, vlr_stream_t stream);
/* out of place through a source-row map: gate | up of row m at row src_rows[m] of gu_src (read only), [d gate | d up] to row m of
 * dgu_out [M][2I], which must not overlap gu_src */
int vlr_swiglu_bwd_src(const void* gu_src, const int* src_rows, void* dgu_out, const void* dact, int M, int I, vlr_stream_t stream);
int vlr_gelu_fwd(const void* z, void* h, long n, vlr_stream_t stream);
int vlr_gelu_bwd(const void* z, const void* dh, void* dz, long n, vlr_stream_t stream);
/* the ViT MLP's activation as a row-wise pass (the layer backward recomputes z and needs h = act(z), dz = dh * act'(z)): act 1 quick-GELU
 * z sigma(1.702 z), act 2 the erf GELU of vlr_gelu_*.  bf16 in / out, fp32 arithmetic, any n >= 1, 16-byte aligned; dz may be dh. */
int vlr_act_fwd(const void* z, void* h, long n, int act, vlr_stream_t stream);
int vlr_act_bwd(const void* z, const void* dh, void* dz, long n, int act, vlr_stream_t stream);
int vlr_colsum_workspace_bytes(int C);
int vlr_colsum(const void* X, int R, int C, int ld, void* out, int accumulate, void* workspace, vlr_stream_t stream);
int vlr_colsum_f32(const void* X, int R, int C, int ld, float* out, void* workspace, vlr_stream_t stream);
int vlr_gather_rows(const void* src, const int* rows, void* dst, int R, int H, vlr_stream_t stream);
int vlr_scatter_rows(const void* src, const int* rows, void* dst, int R, int H, vlr_stream_t stream);
/* The two row copies of the row-compact policy backward (vlr_decoder_layer_bwd_compact; maps: vlr_row_maps below).  bf16 rows of W
 * columns, 16-byte accesses.  Preconditions of both: no null pointer; M / Mc > 0; W > 0 and W % 8 == 0; src, dst 16-byte aligned and
 * not overlapping; every map entry inside its source (dense_own[m] < the rows of src, compact_rows[j] and twin[j] < the rows of src).
 *   vlr_expand_rows_zero: dst [M][W]: dense row m = src row dense_own[m], or zeros where dense_own[m] < 0.
 *   vlr_fold_rows       : dst [Mc][W]: row j = src row compact_rows[j], plus src row twin[j] where twin[j] >= 0 - the sum formed in
 *                         fp32 and rounded to bf16 once (round to nearest even).  One writer per row, fixed order: no atomics. */
int vlr_expand_rows_zero(const void* src, const int* dense_own, void* dst, int M, int W, vlr_stream_t stream);
int vlr_fold_rows(const void* src, const int* compact_rows, const int* twin, void* dst, int Mc, int W, vlr_stream_t stream);
/* strided row-list operations on a column block of a wider matrix (PLoRA of InternLM-XComposer2, reference
 * models/InternLMXC2/build_mlp.py:194-202: `res[im_mask] += Plora_B(Plora_A(x[im_mask]))`):
 *   vlr_rows_gather: dst [R][W] (contiguous) = src[rows[r]][0:W], src row stride lds
 *   vlr_rows_add   : dst[rows[r]][0:W] += src [R][W], dst row stride ldd; `rows` must not repeat */
int vlr_rows_gather(const void* src, int lds, const int* rows, void* dst, int R, int W, vlr_stream_t stream);
int vlr_rows_add(const void* src, const int* rows, void* dst, int ldd, int R, int W, vlr_stream_t stream);
int vlr_cast_f32_to_bf16(const float* src, void* dst, long n, vlr_stream_t stream);
int vlr_cast_bf16_to_f32(const void* src, float* dst, long n, vlr_stream_t stream);
int vlr_rowdot(const void* X, const float* v, float* out, int M, int H, vlr_stream_t stream);

/* ---- attention (transformers LlamaAttention / CLIPAttention, eager semantics: fp32 softmax, causal + key padding
 *      for the decoder, full for the ViT; replaces flash-attn 2.5.8 too, utils/auto_load.py:49-56,534) -------------
 * q/k/v: column blocks of a fused [batch*S][ld] buffer (head h = columns h*head_dim..).  lse: [batch][heads][Sp]
 * floats, Sp = S rounded up to 64, log2 domain.  key_mask: [batch][S] int32 (0 = padded key) or NULL. */
int vlr_attn_fwd(const void* q, const void* k, const void* v, int ld, void* o, int ldo, float* lse,
                 const int* key_mask, int batch, int S, int heads, int head_dim, int causal, float scale,
                 vlr_stream_t stream);
int vlr_attn_bwd(const void* q, const void* k, const void* v, int ld, const void* o, const void* dout, int ldo,
                 const float* lse, float* delta_ws, const int* key_mask, void* dq, void* dk, void* dv, int ldd,
                 int batch, int S, int heads, int head_dim, int causal, float scale, vlr_stream_t stream);

/* grouped-query attention (Mistral / InternLM2: kv_heads < heads; k, v column blocks hold kv_heads heads, query head h reads
 * K/V head h / (heads / kv_heads); dk, dv are summed over the group's query heads in a fixed order - no atomics).
 * vlr_attn_fwd / vlr_attn_bwd are the kv_heads == heads case. */
int vlr_attn_fwd_gqa(const void* q, const void* k, const void* v, int ld, void* o, int ldo, float* lse,
                     const int* key_mask, int batch, int S, int heads, int kv_heads, int head_dim, int causal, float scale,
                     vlr_stream_t stream);
int vlr_attn_bwd_gqa(const void* q, const void* k, const void* v, int ld, const void* o, const void* dout, int ldo,
                     const float* lse, float* delta_ws, const int* key_mask, void* dq, void* dk, void* dv, int ldd,
                     int batch, int S, int heads, int kv_heads, int head_dim, int causal, float scale, vlr_stream_t stream);

/* ---- image/text merge (LlavaForRL._merge_input_ids_with_image_features, Llava/__init__.py:36-109) ---------------
 * info[0] receives the number of image slots found; the caller compares it with n_feat_rows*dup and raises the
 * reference's ValueError (:90-94) on mismatch.  `dup` = how many batch halves share one feature table (the
 * reference duplicates every image, base/trainer.py:138-142; the frozen ViT runs once per distinct image here). */
int vlr_merge_index(const long* input_ids, const long* attention_mask, const long* labels, int Bn, int T, int S, int P,
                    int image_token, int pad_token, int n_feat_rows, int dup, int* src, int* out_mask,
                    long* out_labels, int* out_pos, unsigned char* img_map, int* inv_map, int* info, vlr_stream_t stream);
int vlr_merge_fwd(const int* src, const long* input_ids, const void* embed_table, const void* feats, void* out, int Bn,
                  int T, int S, int H, vlr_stream_t stream);
/* the same into an fp32 residual stream (vlr_llama_cfg.resid_f32): out fp32 [Bn][S][H]; embed_table bf16 (rows widened exactly);
 * feats fp32 [rows][H] when feats_f32 (the projector's unrounded output), else bf16 */
int vlr_merge_fwd_f32(const int* src, const long* input_ids, const void* embed_table, const void* feats, int feats_f32, float* out,
                      int Bn, int T, int S, int H, vlr_stream_t stream);
int vlr_merge_bwd(const void* dmerged, const int* src, const int* inv_map, const long* input_ids, void* dfeats,
                  void* dembed_table, int Bn, int T, int S, int H, int n_feat_rows, int dup, vlr_stream_t stream);
/* NEFTune embedding noise (transformers.trainer_utils.neftune_post_forward_hook: E += U(-m, m), m = alpha / sqrt(T * H), on the output
 * of the input embedding in training mode), in place on the merged x [Bn * S][H] - bf16, or fp32 when x_f32.  Additive entry: the ABI
 * version does not move.  Rows with src[b * S + s] = t >= 0 are text rows (t = the pre-merge token position, the merge's convention):
 * x[c] += n(b * T + t, c).  Image-feature rows and zero rows (src < 0) are neither read nor written - the reference replaces the
 * placeholder rows by image features after the hook ran.  H % 8 == 0.
 *   n: word c % 4 of the Philox4x32-10 block with counter (c / 4, b * T + t, call, pass) and key (low, high half of `key`); its top 24
 *   bits r -> h = r - 8388607.5 (exact), n = h * scale rounded to fp32 once, x + n rounded to fp32 once (no fused multiply-add) and,
 *   for a bf16 x, rounded to nearest-even once more.  scale = m * 2^-23 computed by the caller in fp32, in [0, 1): |n| < m, n != 0
 *   (unless scale is 0), symmetric.  The value depends on (key, call, pass, b * T + t, c) only: a host replay is bit-exact. */
int vlr_neftune_add(void* x, int x_f32, const int* src, int Bn, int T, int S, int H, float scale, uint64_t key, uint32_t call,
                    uint32_t pass, vlr_stream_t stream);

/* ---- log-probabilities (VLDPOTrainer.get_batch_logps, base/trainer.py:148-188) ------------------------------- */
int vlr_build_rows(const long* labels, const unsigned char* shared_mask, int Bn, int S, int label_pad, int* rows,
                   int* tgt, int* seq_off, vlr_stream_t stream);
int vlr_logp_rows(const float* logits, const int* row_idx, const int* tgt, int R, int V, long ld, float* tok_logp,
                  float* lse, vlr_stream_t stream);
int vlr_dlogits_rows(const float* logits, const int* tgt, const float* lse, const int* seq_off, int nseq,
                     const float* dlogps, int average, int R, int V, long ld, void* dlogits, long ldd,
                     vlr_stream_t stream);
int vlr_seq_sum(const float* tok_logp, const int* seq_off, int nseq, int average, float* out, vlr_stream_t stream);
/* Fused lm-head + log-softmax + label pick on the R response rows (SURVEY 8b `vlr_lmhead_logps_fwd/bwd`): hg [R][H] bf16 are the
 * gathered final hidden states, w_lm [V][H]; tok_logp[r] = logit[r][tgt[r]] - lse[r].  When vlr_lmhead_is_fused(R, V, H) the [R][V]
 * logits never reach HBM: the forward GEMM's epilogue leaves per-wave (max, sum exp) partials in `workspace`
 * (vlr_lmhead_workspace_bytes) that a second kernel folds in a fixed order, the backward recomputes the GEMM and writes
 * d logits [R][V] bf16 = g_r * ([v == tgt_r] - softmax) straight from its epilogue (g_r = dlogps of the row's sequence, / row count
 * when `average`).  Otherwise `logits_ws` ([R][V] fp32) carries the logits through vlr_logp_rows / vlr_dlogits_rows. */
long vlr_lmhead_workspace_bytes(int R, int V);
int vlr_lmhead_is_fused(int R, int V, int H);
int vlr_lmhead_logps_fwd(const void* hg, const void* w_lm, const int* tgt, float* tok_logp, float* lse, void* workspace,
                         float* logits_ws, int R, int V, int H, vlr_stream_t stream);
int vlr_lmhead_logps_bwd(const void* hg, const void* w_lm, const int* tgt, const float* lse, const int* seq_off, int nseq,
                         const float* dlogps, int average, void* dlogits, void* workspace, float* logits_ws, int R, int V, int H,
                         vlr_stream_t stream);

/* The same two passes with the POLICY ENTROPY of every row (additive entry points: vlr_abi_version() does not move; what PPO and GRPO
 * log, mask by and regularise with).  H_r = -sum_v p_v log p_v = lse_r - sum_v p_v z_v of row r's softmax, fp32.
 * vlr_lmhead_logps_entropy_fwd: the contract of vlr_lmhead_logps_fwd + entropy [R].  Fused (vlr_lmhead_is_fused, the same predicate):
 *      every wave leaves a TRIPLE per row and 64-column part in `workspace` (vlr_lmhead_entropy_workspace_bytes) - (m, s, t) with m the
 *      part's maximum, s = sum e^(z - m), t = sum e^(z - m) (z - m) over the part's columns < V (every term of t is <= 0: nothing
 *      cancels) - and the lane that owns the target column stores the raw target logit.  A second kernel folds the parts of a row in a
 *      fixed order, without atomics: M = max m_i, S = sum s_i e^(m_i - M), T = sum e^(m_i - M) (t_i + (m_i - M) s_i), lse = M + log S,
 *      H = log S - T / S.  tok_logp and lse are BIT-IDENTICAL to vlr_lmhead_logps_fwd on the same inputs (the same partial maxima and
 *      sums, the same fold order): a caller switches entropy on without moving a log-prob.  Otherwise `logits_ws` ([R][V] fp32)
 *      carries the logits through vlr_logp_ent_rows, which walks a row in vlr_logp_rows's order (the same bit-equality).
 * vlr_lmhead_logps_entropy_bwd: dlogp and dent are per-row fp32 [R] (no seq_off: one row per "sequence"); with p = exp(z - lse_r)
 *      dlogits[r][v] = bf16(dlogp_r ([v == tgt_r] - p) - dent_r (p ((z - lse_r) + H_r))), the parentheses give the order of
 *      evaluation, rounded once, 16-byte stores.  d H_r / d z_v = -p_v (log p_v + H_r).  Where the second product is zero the first
 *      term is stored as it is, so with dent all zero the result is BIT-IDENTICAL to vlr_lmhead_logps_bwd(nseq = R, seq_off = 0..R,
 *      average = 0), the sign of a zero included.  `workspace` non-NULL selects the fused route where it applies (it is not written);
 *      otherwise `logits_ws` and vlr_dlogits_ent_rows. */
long vlr_lmhead_entropy_workspace_bytes(int R, int V);
int vlr_lmhead_logps_entropy_fwd(const void* hg, const void* w_lm, const int* tgt, float* tok_logp, float* lse, float* entropy,
                                 void* workspace, float* logits_ws, int R, int V, int H, vlr_stream_t stream);
int vlr_lmhead_logps_entropy_bwd(const void* hg, const void* w_lm, const int* tgt, const float* lse, const float* entropy,
                                 const float* dlogp, const float* dent, void* dlogits, void* workspace, float* logits_ws, int R, int V,
                                 int H, vlr_stream_t stream);
int vlr_logp_ent_rows(const float* logits, const int* tgt, int R, int V, long ld, float* tok_logp, float* lse, float* entropy,
                      vlr_stream_t stream);
int vlr_dlogits_ent_rows(const float* logits, const int* tgt, const float* lse, const float* entropy, const float* dlogp,
                         const float* dent, int R, int V, long ld, void* dlogits, long ldd, vlr_stream_t stream);

/* ---- supervised fine-tuning: the causal-LM cross-entropy `loss` of the model wrappers' forward(labels=...) (reference
 *      Llava/__init__.py:246-257, LlavaNext/__init__.py:322-331, modeling_qwen.py:839-842, InternLMXC2/__init__.py:211-219) = the mean of
 *      -log p(label) over the selected rows of the WHOLE batch, on the tok_logp / lse of vlr_lmhead_logps_fwd.
 * vlr_ce_mean_fwd: out3 = {loss = -sum_r tok_logp[r] / R, R, -1/R}.  Per-block partials, then one fold, in an order that depends on R
 *      only and without atomics: two calls are bit-equal.  workspace: vlr_ce_mean_workspace_bytes().
 * vlr_lmhead_ce_bwd: d hg [R][H] bf16 and (dw_lm != NULL) d W_lm [V][H] bf16 (+= when dw_accumulate) for the uniform row gradient
 *      *coef (device scalar: upstream gradient x out3[2]).  The rows are walked in blocks of at most `row_block` rows (<= 0: the
 *      default, vlr_lmhead_ce_row_block: the largest multiple of 256 that keeps the block's workspace under 1 GiB) - per block
 *      vlr_lmhead_logps_bwd into `dlogits` [row_block][V] bf16, then the dgrad and wgrad GEMMs.  `workspace`:
 *      vlr_lmhead_workspace_bytes(row_block, V); `logits_ws` fp32 [rows][V] for every block size that is not vlr_lmhead_is_fused.
 *      d hg is computed row by row from operands of that row alone, so it is bit-identical for every block size as long as the blocks
 *      reach the same GEMM kernels (the dispatcher picks tiles by the row count).  d W_lm is NOT: it sums over the rows, each block's
 *      product is rounded to bf16 when it is added to the gradient buffer, in block order - deterministic for a given row_block,
 *      equal to the single-block result only to bf16 rounding. */
int vlr_ce_mean_workspace_bytes(void);
int vlr_ce_mean_fwd(const float* tok_logp, int R, void* workspace, float* out3, vlr_stream_t stream);
int vlr_lmhead_ce_row_block(int R, int V, int H);
int vlr_lmhead_ce_bwd(const void* hg, const void* w_lm, const int* tgt, const float* lse, const float* coef, void* dlogits,
                      void* workspace, float* logits_ws, void* dhg, void* dw_lm, int dw_accumulate, int R, int V, int H, int row_block,
                      vlr_stream_t stream);

/* ---- reward-model head (reference base/model.py VLRewardModel: rm_head = nn.Linear(hidden, 1) on hidden_states[-1][:, -1, :]; additive
 *      entry points, vlr_abi_version() does not move).  hidden [*][ldh] bf16 = the final hidden states, rows[i] the row of reward i,
 *      w [H] bf16, b [1] bf16.  H % 8 == 0, H >= 8, ldh / ldd multiples of 8 (16-byte loads).  No atomics.
 * vlr_rm_head_fwd: rewards[i] = dot(hidden[rows[i]], w) + b, accumulated and written in fp32 (never rounded to bf16).  One workgroup per
 *      row with a fixed reduction order: a row's reward has the same bits for every n and from call to call.
 * vlr_rm_head_bwd: dhidden[rows[i]] = bf16(d_rewards[i] * w) - no other row of dhidden is touched (the caller zeroes it), `rows` must
 *      not repeat; dw[h] = sum_i d_rewards[i] * hidden[rows[i]][h] and db = sum_i d_rewards[i], both in fp32 in the order of i and
 *      rounded once into the bf16 gradient buffers - with `accumulate` the old value is added in fp32 before that one rounding.
 * The pair loss -logsigmoid(r_chosen - r_rejected) is vlr_dpo_loss(beta 1, label_smoothing 0, loss_type 0, reference_free 1). */
int vlr_rm_head_fwd(const void* hidden, int ldh, const int* rows, const void* w, const void* b, float* rewards, int n, int H,
                    vlr_stream_t stream);
int vlr_rm_head_bwd(const void* hidden, int ldh, const int* rows, const void* w, const float* d_rewards, void* dhidden, int ldd,
                    void* dw, void* db, int accumulate, int n, int H, vlr_stream_t stream);

/* ---- PPO (reference ppo.py / VLPPOTrainer, whose step is trl 0.8.1's PPOTrainer.step; additive entry points, vlr_abi_version() does
 *      not move).  Every per-token tensor is compact [R] fp32 over the response rows of vlr_build_rows (the rows whose logits predict a
 *      response token; the values are read on the same rows), seq_off [n + 1] delimits the n sequences.  No atomics: every reduction
 *      runs in an order fixed by the sizes alone, two calls give the same bits.  exp is expf.
 * vlr_ppo_advantages: kl_t = old_logp - ref_logp (kl_penalty 0 "kl"), |.| (1 "abs"), 0.5 (.)^2 (2 "mse"); reward_t = -kl_coef kl_t, the
 *      last token of sequence s gets + scores[s]; whiten_rewards: rewards <- masked_whiten(rewards, shift_mean = False) over all R
 *      tokens.  Per sequence, backwards: delta_t = r_t + gamma V_{t+1} - V_t (V past the end = 0), A_t = delta_t + gamma lam A_{t+1},
 *      returns = A + V; then advantages <- masked_whiten(A) over all R tokens.  masked_whiten(x) = (x - mean) / sqrt(var + 1e-8) with
 *      var = the biased variance x R / (R - 1); shift_mean = False adds the mean back.  kl_sums[s] = sum_t kl_t; stats[4] = {mean of
 *      kl_sums over the sequences, mean non-score reward per token, mean and (R / (R - 1)) variance of A before whitening}.
 *      R >= 2 (refused before any launch), 1 <= n <= R.  One workgroup of 1024 threads: wave per sequence for the rewards, thread
 *      per sequence for the scan, thread-strided sums folded by xor butterflies and the 16 waves in order.
 * vlr_ppo_loss: ratio = exp(logp - old_logp); pg = mean(max(-A ratio, -A clamp(ratio, 1 - cliprange, 1 + cliprange)));
 *      vf = 0.5 mean(max((vpred - ret)^2, (clamp(vpred, V_old - cliprange_value, V_old + cliprange_value) - ret)^2));
 *      loss = pg + vf_coef vf; means are sums over the R tokens / R.  dlogp / dvpred = upstream * d loss / d logp, d vpred exactly as
 *      torch autograd differentiates that expression (clamp passes the gradient on its closed interval, max halves a tie), final on
 *      return.  mean(ratio) > ratio_threshold: pg, vf, loss and every gradient are exactly 0, decided on the device.  The ratio bounds
 *      are formed in double and rounded to fp32 once (torch.clamp with Python floats); V_old -+ cliprange_value in fp32.
 *      stats[17] = {loss, pg, vf, approxkl = 0.5 mean((logp - old)^2), policykl = mean(old - logp), pg_clipfrac, vf_clipfrac (both
 *      strict >), mean ratio, returns mean, returns var, vpred mean, vpred var, value error = mean((vpred - ret)^2), advantages mean,
 *      old values mean, old values var, 1 when the ratio threshold tripped}; variances as masked_var (x R / (R - 1)).  R >= 2.
 *      One workgroup of 1024 threads: the threshold needs the mean over all tokens before any gradient is written.
 * vlr_v_head_bwd: the value head v_r = dot(hg[r], w) + b on ALL R gathered rows hg [R][H] bf16 (its forward is vlr_rm_head_fwd with
 *      rows = 0..R-1, ldh = H).  dhg_inout[r] = bf16(float(dhg_inout[r]) + g_r w): added onto the lm-head backward's gathered d hg,
 *      rows >= R untouched; dw[h] = sum_r g_r hg[r][h], db = sum_r g_r in fp32, rounded to bf16 once - with `accumulate` the old value
 *      is added in fp32 before that rounding.  The rows are cut into ceil(R / max(8, ceil(R / 256))) chunks, one wave per chunk and
 *      64 column groups, the chunk partials (fp32, in `workspace`: vlr_v_head_bwd_workspace_bytes(R, H)) are folded in chunk order by a
 *      second kernel.  H % 8 == 0, H >= 8, R >= 1. */
int vlr_ppo_advantages(const float* old_logp, const float* ref_logp, const float* values, const int* seq_off, const float* scores,
                       float kl_coef, int kl_penalty, float gamma, float lam, int whiten_rewards, float* advantages, float* returns,
                       float* kl_sums, float* stats, int R, int n, vlr_stream_t stream);
int vlr_ppo_loss(const float* logp, const float* vpred, const float* old_logp, const float* old_values, const float* advantages,
                 const float* returns, int R, double cliprange, double cliprange_value, float vf_coef, float ratio_threshold,
                 float upstream, float* dlogp, float* dvpred, float* stats, vlr_stream_t stream);
long vlr_v_head_bwd_workspace_bytes(int R, int H);
int vlr_v_head_bwd(const void* hg, const void* w, const float* g, void* dhg_inout, void* dw, void* db, int accumulate, void* workspace,
                   int R, int H, vlr_stream_t stream);

/* ---- GRPO (Group Relative Policy Optimization: G samples per prompt, the advantage is the reward standardised inside its group; no
 *      value head, no GAE, no whitening across the batch; additive entry points, vlr_abi_version() does not move).  As for PPO: the
 *      per-token tensors are compact [R] fp32 over the response rows of vlr_build_rows, seq_off [n + 1] delimits the n sequences, no
 *      atomics, every reduction runs in an order fixed by the sizes alone (two calls give the same bits), exp is expf, nothing allocates.
 * vlr_grpo_advantages: scores [P * G], row p G + j is sample j of prompt p.  Per group: mean_p = sum_j s / G, std_p = sqrt(sum_j
 *      (s - mean_p)^2 / (G - 1)) (unbiased, torch.std), A = (s - mean_p) / (std_p + 1e-4) when scale_rewards, else s - mean_p.  The
 *      moments are taken of the scores shifted by the group's first one, so a group of equal scores gives std_p = 0 and A = 0 exactly,
 *      never NaN.  stats[4] = {mean of all scores, mean over the groups of std_p, fraction of groups with std_p == 0, 0}.
 *      P >= 1, G >= 2 (refused before any launch).  One workgroup of 1024 threads: wave per group, lane-strided sums folded by xor
 *      butterflies, the statistics summed per wave in group order and over the 16 waves in order.
 * vlr_grpo_loss: for token t of sequence s, with A = adv_seq[s]: r = exp(logp - old_logp),
 *      l = -min(r A, clamp(r, 1 - eps_low, 1 + eps_high) A), and when beta != 0, with d = ref_logp - logp: l += beta (exp(d) - d - 1).
 *      loss_type 0 "grpo": (1 / n) sum_s (1 / len_s) sum_t l; 1 "bnpo": sum l / R; 2 "dr_grpo": sum l / (n max_completion_length).
 *      old_logp NULL stands for logp itself with the gradient stopped: the ratio is exactly 1 and the gradient still flows.  ref_logp
 *      may be NULL only when beta == 0 (it is not read then).  The bounds 1 - eps_low and 1 + eps_high are formed in double and rounded
 *      to fp32 once (torch.clamp with Python floats).  dlogp = upstream * d loss / d logp exactly as torch autograd differentiates that
 *      expression (clamp passes the gradient on its closed interval, min halves a tie): -A r inside the clip range and where the
 *      unclipped branch is the smaller one, 0 on the clipped side; final on return.  stats[8] = {loss, token-mean of the KL term (0 when
 *      beta == 0), clip fraction low (r < 1 - eps_low and A < 0), clip fraction high (r > 1 + eps_high and A > 0), their sum, mean
 *      ratio, mean len_s = R / n, 0}; the fractions and means are over the R tokens.  R >= 1, 1 <= n <= R, eps >= 0, loss_type in
 *      0..2, max_completion_length >= 1 for loss_type 2 (read by no other).  One workgroup of 1024 threads, one pass: wave per
 *      sequence (a token finds its sequence without a search), lanes stride its tokens. */
int vlr_grpo_advantages(const float* scores, int P, int G, int scale_rewards, float* advantages, float* stats, vlr_stream_t stream);
int vlr_grpo_loss(const float* logp, const float* old_logp, const float* ref_logp, const float* adv_seq, const int* seq_off, int R, int n,
                  double eps_low, double eps_high, float beta, int loss_type, int max_completion_length, float upstream, float* dlogp,
                  float* stats, vlr_stream_t stream);

/* vlr_grpo_loss_ent: vlr_grpo_loss with the policy entropy of every token (additive entry point).  entropy [R] fp32 (H_t of
 *      vlr_lmhead_logps_entropy_fwd), keep [R] bytes (0 / 1; NULL = every token kept: trl's top_entropy_quantile mask), entropy_coef:
 *      l_t = keep_t (clipped surrogate + beta KL term) - entropy_coef H_t.  The normaliser of every loss_type is vlr_grpo_loss's:
 *      "grpo" still divides by the full len_s, as trl does when it masks by entropy.  dlogp = vlr_grpo_loss's gradient x keep_t;
 *      dent_t = -entropy_coef x upstream x (token t's normaliser weight: 1 / (n len_s), 1 / R or 1 / (n max_completion_length)).
 *      stats[10]: [0..7] as vlr_grpo_loss ([0] the loss above), [8] the token-mean of H, [9] the fraction of tokens kept.  stats[1..5]
 *      (KL mean, clip fractions, mean ratio) REMAIN MEANS OVER ALL R TOKENS, kept or not.  entropy may be NULL when entropy_coef == 0
 *      (H reads as 0, stats[8] = 0).  With keep = NULL and entropy_coef = 0, dlogp and stats[0..7] are vlr_grpo_loss's bits.  The same
 *      single workgroup, wave per sequence and fixed reduction orders. */
int vlr_grpo_loss_ent(const float* logp, const float* old_logp, const float* ref_logp, const float* adv_seq, const int* seq_off, int R,
                      int n, double eps_low, double eps_high, float beta, int loss_type, int max_completion_length, float upstream,
                      const float* entropy, const unsigned char* keep, float entropy_coef, float* dlogp, float* dent, float* stats,
                      vlr_stream_t stream);

/* ---- KTO (Kahneman-Tversky Optimization on UNPAIRED feedback: trl's KTOTrainer.kto_loss; additive entry point, vlr_abi_version() does
 *      not move).  A main row is one prompt, one completion and one label (1 desirable, 0 undesirable); a KL row is a prompt with another
 *      row's completion.  Every input is a SUMMED completion log-prob: pi / ref [n] fp32 of the policy and the reference on the main rows,
 *      label [n] bytes, pi_kl / ref_kl [m] fp32 on the KL rows.
 *      kl     = max(0, (1 / m) sum_j (pi_kl[j] - ref_kl[j]))      a constant: no gradient flows into it (trl detaches it)
 *      r_i    = pi[i] - ref[i]
 *      loss_i = w_desirable   (1 - sigmoid(beta (r_i - kl)))      label[i] != 0
 *             = w_undesirable (1 - sigmoid(beta (kl - r_i)))      label[i] == 0
 *      loss   = (1 / n) sum_i loss_i                              over ALL n rows, whichever labels occur
 *      rewards[i] = beta r_i
 *      dpi[i] = upstream d loss / d pi[i] = -(w_desirable beta / n) s (1 - s) upstream,   s = sigmoid(beta (r_i - kl))    label != 0
 *                                         = +(w_undesirable beta / n) s (1 - s) upstream, s = sigmoid(beta (kl - r_i))    label == 0
 *      The weight is formed on the host in fp32 as ((w beta) / n) upstream.  1 - sigmoid(z) is computed as 1 / (1 + expf(z)): a
 *      saturated z gives loss_i = w or 0 and dpi[i] = 0 exactly, never NaN; z = 0 gives loss_i = w / 2 and s (1 - s) = 1 / 4 exactly.
 *      losses, rewards, dpi [n] fp32, final on return.  stats[8] = {loss, kl, sum of rewards over label 1, over label 0, sum of pi over
 *      label 1, over label 0, count of label 1, count of label 0}.
 *      Refused before any launch: a null pointer, n or m outside 1 .. 2^20, beta, a weight or upstream that is not finite.  One
 *      workgroup of 1024 threads whose lanes stride the rows; every sum is per-lane partials, six xor butterflies, then the 16 waves in
 *      order: no atomics, two calls give the same bits; exp is expf; nothing allocates. */
int vlr_kto_loss(const float* pi, const float* ref, const unsigned char* label, int n, const float* pi_kl, const float* ref_kl, int m,
                 float beta, float w_desirable, float w_undesirable, float upstream, float* losses, float* rewards, float* dpi,
                 float* stats, vlr_stream_t stream);

/* ---- sampling: the next token of every row of a generate batch, chosen on the device (additive entry point, vlr_abi_version() does
 *      not move).  One launch per new token on the fp32 logits the lm-head left in HBM; nothing allocates, the logits are never written.
 * vlr_sample_tokens: logits [B][ld] fp32 (ld >= V, 1 <= V < 2^24).  Per row r with unfinished[r] != 0, in this order:
 *   1. repetition penalty (transformers RepetitionPenaltyLogitsProcessor; repetition_penalty > 0, 1 = none): every id of the row's
 *      history - the T ids of prompt row r / prompt_div of prompt_ids [ceil(B / prompt_div)][prompt_ld] int64, pads included as
 *      transformers does, and the first n_gen columns of row r of gen_ids [B][gen_ld] int64 - gets z = z < 0 ? z * pen : z / pen, ONCE
 *      however often it occurs (a V-bit membership map in LDS: V <= 2^19 with a penalty; ids outside [0, V) are ignored).
 *   2. temperature (> 0), when do_sample: z = z / temperature, an fp32 division.  1 and 2 are single correctly rounded fp32 operations.
 *   3. top-k, when do_sample and 0 < top_k < V: keep z >= the k-th largest z; everything tied with the k-th is kept.
 *   4. top-p, when do_sample and top_p < 1 (top_p in (0, 1]): over the survivors of 3, p = softmax(z); a token is kept iff the mass of
 *      the tokens with STRICTLY greater z is < top_p.  This is transformers' TopPLogitsWarper (min_tokens_to_keep = 1) wherever no tie
 *      straddles the cut, and keeps the whole tie group where one does (transformers cuts through it in sort order).
 *   5. the draw, Gumbel-max over the kept set: tok = argmax_i (z_i + g_i), the lowest index on an exact tie; g_i = -log(-log u_i),
 *      u_i = ((w_i >> 8) + 1/2) 2^-24, w_i = word i % 4 of Philox4x32-10 with the counter (i / 4, row_id, step, call) and the two halves
 *      of `seed` as its key (low half first); row_id = row_ids[r], or r when row_ids is NULL.  A draw depends on (seed, call, row_id,
 *      step, i) alone - not on B, the row's place in the launch or any reduction order.  The 24-bit uniform truncates the Gumbel
 *      variate at +17.33 and -2.85 (a token whose probability is below e^-20 of the mode's is never drawn), which is the second
 *      deliberate difference from transformers' inverse-CDF torch.multinomial.  Greedy (do_sample = 0): tok = argmax z after step 1
 *      only, the lowest index on ties, the kept set is every column, no random numbers.
 *   6. logp[r] = z_tok - logsumexp(z over the kept set): the score of transformers' compute_transition_scores.
 *   7. next_tok[r] = tok (int32: what the decode step consumes) and out_ids[r * out_ld + step] = tok (int64: the caller's ids, which
 *      may be gen_ids itself - history columns are read before the write); when tok is one of the n_eos <= 8 ids of eos_ids (device,
 *      int32): unfinished[r] = 0 and finish_step[r] = step.  The eos itself is emitted.
 *   A row with unfinished[r] == 0 gets pad in both places and logp 0, draws nothing, and its flags and kept row stay as they are.
 *   kept (NULL in production; [B][V] bytes): 1 where the column survived the warpers, else 0.
 *   One workgroup of 1024 threads per row; thresholds by 16-way bisection on the order-preserving integer image of z (counts for
 *   top-k, masses for top-p: up to 9 passes over the row each, no sort, no workspace).  No floating-point atomics: every float sum
 *   runs per thread over its 4-column groups in ascending order, then six xor butterflies, then the 16 waves in order - fixed by V and
 *   the geometry, so two calls give the same bits.  Rows must hold at least one finite logit and no NaN.  Argument ranges are refused
 *   before any launch. */
int vlr_sample_tokens(const float* logits, int B, int V, int ld, int do_sample, float temperature, int top_k, float top_p,
                      float repetition_penalty, const int64_t* prompt_ids, int T, int prompt_ld, int prompt_div, const int64_t* gen_ids,
                      int gen_ld, int n_gen, const int* eos_ids, int n_eos, int pad, uint64_t seed, uint32_t call, uint32_t step,
                      const int* row_ids, unsigned char* unfinished, int* next_tok, int64_t* out_ids, int out_ld, float* logp,
                      int* finish_step, unsigned char* kept, vlr_stream_t stream);

/* ---- DPO loss, forward + backward (VLDPOTrainer.dpo_loss, base/trainer.py:244-301).
 * loss_type 0 sigmoid|ddpo, 1 hinge, 2 ipo, 3 kto_pair (losses has 2n entries).  dpc/dpr = d(sum_i g_i*loss_i)/d
 * policy_{chosen,rejected}_logps with g = grad_losses or 1/len(losses) when NULL (trl: loss = losses.mean()). */
int vlr_dpo_loss(const float* pc, const float* pr, const float* rc, const float* rr, int n, float beta,
                 float label_smoothing, int loss_type, int reference_free, float* losses, float* chosen_rewards,
                 float* rejected_rewards, float* dpc, float* dpr, float* loss_mean, const float* grad_losses,
                 vlr_stream_t stream);

/* ---- optimizer on flat buffers (torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW as driven by the HF Trainer;
 *      hyper-parameters scripts/dpo_llava.sh:35-41).  out3 = {grad norm, clip coefficient * gscale, raw sum g^2};
 *      vlr_adamw_step reads coef[1] on the device (no host sync). */
int vlr_grad_sqnorm_workspace_bytes(void);
int vlr_grad_sqnorm(const void* grads, long n, float max_norm, float gscale, float extra_sq, void* workspace,
                    float* out3, vlr_stream_t stream);
int vlr_adamw_step(float* master, float* m, float* v, const void* grads, void* params_bf16, long n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, const float* coef,
                   vlr_stream_t stream);

/* ---- composed passes (transformers LlamaDecoderLayer / CLIPEncoderLayer forward + autograd backward) ---------- */
typedef struct {
    int hidden, inter, heads, head_dim;
    float rms_eps;
    int max_pos;            /* rows of the rope tables */
    const float* rope_cos;  /* [max_pos][head_dim/2] */
    const float* rope_sin;
    int kv_heads;           /* grouped-query attention (Mistral, InternLM2): K/V heads, a divisor of heads; 0 = heads */
    int resid_f32;          /* 1: the residual stream (x_in, acts.x_mid, acts.x_out) is fp32 [M][hidden] - never rounded to bf16; the
                             * norms read it in fp32, o_proj / down_proj add their fp32 accumulators to it (vlr_gemm_bf16_f32res).
                             * HF runs the bf16 checkpoint's residual adds in bf16 (transformers LlamaDecoderLayer.forward); this mode
                             * is what brings the 32-layer loss within north_star's tolerance of the fp32 reference.  The gradient
                             * stream (dx_out / dx_in) stays bf16.  0: bf16 stream (ABI v3 behaviour) */
} vlr_llama_cfg;
/* Shapes with Nq = heads*head_dim, Nkv = kv_heads*head_dim: wqkv [Nq + 2 Nkv][hidden] (q | k | v rows), wo [hidden][Nq],
 * qkv / dqkv activations [M][Nq + 2 Nkv], attn / dattn [M][Nq].  hidden == Nq for LLaMA / Mistral. */
typedef struct {  /* bf16 weights of one decoder layer; q|k|v and gate|up are stored fused */
    const void* ln1; const void* wqkv; const void* wo; const void* ln2; const void* wgu; const void* wdown;
    const void* bqkv;       /* [Nq + 2 Nkv] bias of the fused q|k|v projection (Qwen c_attn, QwenVL/modeling_qwen.py:104); NULL = none.
                             * Its gradient is the column sum of the dqkv scratch after vlr_decoder_layer_bwd (vlr_colsum). */
} vlr_layer_weights;
typedef struct {  /* bf16 gradient buffers, same shapes */
    void* ln1; void* wqkv; void* wo; void* ln2; void* wgu; void* wdown;
} vlr_layer_grads;
typedef struct {  /* activations one layer keeps for its backward (caller-allocated) */
    void* xn1; float* rstd1; void* qkv; void* attn; float* lse; void* x_mid; void* xn2; float* rstd2; void* gu;
    void* act; void* x_out;
} vlr_layer_acts;
typedef struct {  /* scratch shared by all layers in the backward */
    void* dact; void* dxn; void* dattn; void* dqkv; void* dx_mid; float* delta; void* norm_ws;
} vlr_layer_bwd_ws;

int vlr_decoder_layer_fwd(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_acts* a,
                          const void* x_in, const int* pos, const int* key_mask, int batch, int S,
                          vlr_stream_t stream);
/* keep_for_backward = 0: a no-grad pass (reference model, evaluation) - tensors only the backward reads are not written */
int vlr_decoder_layer_fwd_ex(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_acts* a,
                             const void* x_in, const int* pos, const int* key_mask, int batch, int S,
                             int keep_for_backward, vlr_stream_t stream);
/* Row-compact no-grad layer (additive entry point: vlr_abi_version() does not move).  A DPO batch is [chosen ; rejected] and the two
 * sequences of a pair share their prompt (and image): attention is causal and every other operator of the layer is row-wise, so in
 * every layer the rejected sequence's prompt rows repeat the chosen sequence's.  The caller keeps Mc <= batch * S rows:
 *   compact_rows [Mc]         int32, ascending: the dense row (b * S + s) each kept row stands at;
 *   dense_src    [batch * S]  int32: for every dense row the kept row that holds its value (a dropped row names its twin), < Mc;
 *   pos_compact  [Mc]         the positions of the kept rows.
 * x_in and every tensor of `a` hold Mc rows, except a->lse, which stays [batch][heads][align64(S)].  qkv_dense [batch * S][Nq + 2 Nkv]
 * and attn_dense [batch * S][Nq] are scratch: the q|k|v rows are expanded through dense_src, vlr_attn_fwd_gqa runs on the dense
 * layout with the dense key_mask exactly as in vlr_decoder_layer_fwd_ex, and its rows are compacted again through compact_rows.
 * (Where the persistent kernel takes o_proj with a row map it reads those dense rows through compact_rows instead, and a->attn is not
 * written.)  keep_for_backward = 0 semantics (a->gu is not written).
 * tail_rows: how many of the LAST dense rows are kept (the compact rows Mc - tail_rows .. Mc - 1 are the dense rows
 * batch * S - tail_rows .. batch * S - 1).  The residual projections of the dense pass run their last vlr_gemm_peel_rows(batch * S, hidden)
 * rows on the 128x128 split-K kernel, whose fp32 sums are formed in another order than the persistent kernel's; when these rows lie
 * inside the kept tail the compact pass peels exactly them, every row is computed by the kernel the dense pass computes it in, and
 * the kept rows of x_out equal vlr_decoder_layer_fwd_ex's bit for bit.  Otherwise the launches split as their own row count suggests
 * and rows near the end may differ in their fp32 summation order. */
int vlr_decoder_layer_fwd_compact(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_acts* a, const void* x_in,
                                  const int* pos_compact, const int* dense_src, const int* compact_rows, int Mc, int tail_rows,
                                  void* qkv_dense, void* attn_dense, const int* key_mask, int batch, int S, vlr_stream_t stream);
/* rows the plain GEMM launch of [M x N] (vlr_gemm_bf16, vlr_gemm_bf16_f32res) hands to the 128x128 split-K kernel: its last rows; 0: none */
int vlr_gemm_peel_rows(int M, int N);
int vlr_decoder_layer_bwd(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_grads* g,
                          int accumulate, const vlr_layer_acts* a, const vlr_layer_bwd_ws* ws, const void* x_in,
                          const void* dx_out, void* dx_in, const int* pos, const int* key_mask, int batch, int S,
                          vlr_stream_t stream);

/* ---- the row-compact POLICY pass: forward kept for a backward, and that backward (additive: vlr_abi_version() does not move) ----
 * The maps of one [chosen ; rejected] batch, device int32 arrays (vlrlhf/prefix_dedup.py build_policy_plan), M = batch * S:
 *   compact_rows [Mc], dense_src [M], pos_compact [Mc]   as for vlr_decoder_layer_fwd_compact;
 *   dense_own [M]   the kept row of a KEPT dense row, -1 for a dropped row;
 *   twin [Mc]       the dense index of the dropped twin of a shared kept row, -1 for a row that stands for itself alone. */
typedef struct {
    const int* compact_rows; const int* dense_src; const int* dense_own; const int* twin; const int* pos_compact;
    int Mc, tail_rows;
} vlr_row_maps;
typedef struct {  /* dense scratch of the attention section, [batch * S] rows each: qkv, dqkv [.][Nq + 2 Nkv]; attn, dattn [.][Nq] */
    void* qkv; void* attn; void* dattn; void* dqkv;
} vlr_dense_scratch;
/* vlr_decoder_layer_fwd_compact with keep_for_backward: 1 writes a->gu as vlr_decoder_layer_fwd_ex does; 0 is
 * vlr_decoder_layer_fwd_compact itself (which forwards here).  What the pass keeps - every tensor of `a` but a->lse - holds Mc rows.
 * Preconditions: no null pointer but key_mask; 0 < Mc <= batch * S; 0 <= tail_rows <= Mc; heads % kv_heads == 0; the maps as
 * described above; every buffer sized as stated there; nothing is allocated. */
int vlr_decoder_layer_fwd_compact_ex(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_acts* a, const void* x_in,
                                     const int* pos_compact, const int* dense_src, const int* compact_rows, int Mc, int tail_rows,
                                     void* qkv_dense, void* attn_dense, const int* key_mask, int batch, int S, int keep_for_backward,
                                     vlr_stream_t stream);
/* The same pass with the maps as a struct.  Where m->twin is given and the fused kernels take every row of the layer's shapes (head_dim
 * 128, the 7B widths) the q|k|v + RoPE epilogue stores each kept row straight to its row of qkv_dense and a shared row to its dropped
 * copy's too (vlr_gemm_qkv_rope_bias_dst): no row copy rebuilds the dense q|k|v and a->qkv is not written.  Elsewhere, and with
 * m->twin == NULL, it is vlr_decoder_layer_fwd_compact_ex call for call.  Every value written equals that function's, bit for bit.
 * m->dense_own is not read.  keep_for_backward = 0: the no-grad reference pass (vlr_decoder_layer_fwd_compact). */
int vlr_decoder_layer_fwd_compact_maps(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_acts* a, const void* x_in,
                                       const vlr_row_maps* m, void* qkv_dense, void* attn_dense, const int* key_mask, int batch, int S,
                                       int keep_for_backward, vlr_stream_t stream);
/* The activations that pass left on Mc rows (`c`), copied to the dense layout (`d`: batch * S = M rows) through dense_src, so that the
 * unchanged vlr_decoder_layer_bwd runs on `d` and computes what it computes after a dense forward - the same bits wherever
 * vlr_decoder_layer_compact_exact says 1.  Copied: x_out, and with keep_for_backward = 1 also xn1, rstd1, x_mid, xn2, rstd2, gu, act.
 * NOT copied: q|k|v, attn, lse - give the compact forward d->qkv and d->attn as its dense scratch and set c->lse = d->lse.
 * Preconditions: no null pointer among the copied tensors; M > 0; dense_src[m] < Mc for every m; hidden % 8 == 0 and inter % 8 == 0;
 * `c` and `d` do not overlap; nothing is allocated.  vlr_gather_f32: dst[i] = src[idx[i]], n > 0 fp32 values (the rstd copies). */
int vlr_layer_acts_expand(const vlr_llama_cfg* cfg, const vlr_layer_acts* c, const vlr_layer_acts* d, const int* dense_src, int M,
                          int keep_for_backward, vlr_stream_t stream);
int vlr_gather_f32(const float* src, const int* idx, float* dst, int n, vlr_stream_t stream);
/* The adjoint of that pass: vlr_decoder_layer_bwd with every row-wise call at Mc rows, in the same order.  x_in, dx_out, dx_in, the
 * tensors of `a` (a->lse excepted) and of `ws` (ws->delta excepted: [batch][heads][align64(S)]) hold Mc rows.  The attention backward
 * alone runs densely: d attn is expanded with zeros on the dropped rows (no gradient enters there: their delta and dS are exactly 0),
 * q|k|v and attn are expanded through dense_src, the unchanged vlr_attn_bwd_gqa runs on [batch * S] rows, and d qkv is folded - a shared
 * row receives its own gradient plus what the rejected response rows sent to the dropped copy's keys and values; that one bf16 sum is
 * the only rounding the dense backward does not have.  ws->dqkv holds the folded d qkv [Mc] afterwards (its column sum is the gradient
 * of a q|k|v bias).
 * Preconditions: no null pointer but key_mask, in the structs too; 0 < m->Mc <= batch * S; heads % kv_heads == 0;
 * hidden % 8 == 0, (Nq + 2 Nkv) % 8 == 0 and Nq % 8 == 0 (the row copies); nothing is allocated.  The weight-gradient GEMMs contract
 * over the kept rows: Mc % 8 == 0 lets dW_gate|up and dW_down share one launch (vlr_gemm_bf16_tn_pair), as in the dense backward. */
int vlr_decoder_layer_bwd_compact(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_grads* g, int accumulate,
                                  const vlr_layer_acts* a, const vlr_layer_bwd_ws* ws, const vlr_row_maps* m,
                                  const vlr_dense_scratch* d, const void* x_in, const void* dx_out, void* dx_in, const int* key_mask,
                                  int batch, int S, vlr_stream_t stream);
/* ---- the dense backward on the kept rows IN PLACE (additive: vlr_abi_version() does not move).  vlr_layer_acts_expand buys the dense
 * layout back with eight row copies per layer; five of them feed consumers that walk rows one at a time and can read row m at
 * src[dense_src[m]] instead.
 * vlr_decoder_layer_fwd_compact_keep: vlr_decoder_layer_fwd_compact_ex(keep_for_backward = 1) writing
 *   - rstd1, x_mid, rstd2, gu, x_out on Mc rows into the layer's own set `a` (never copied),
 *   - xn1, xn2, act (the K-side operands of the weight-gradient GEMMs) and q|k|v straight to the M dense rows of `a` where the fused
 *     kernels take every row of the layer's shapes: the scatter norms (vlr_rmsnorm_fwd_scatter) and the output maps of the two fused
 *     epilogues (vlr_gemm_qkv_rope_bias_dst, vlr_gemm_swiglu_dst) store a shared row to both of its dense rows, the projections read
 *     xn1 / xn2 through compact_rows and down_proj reads act the same way (vlr_gemm_res_rows).  No row is copied; s->xn1, s->qkv,
 *     s->xn2 and s->act are NOT written on this route,
 *   - elsewhere (toy widths; act also where down_proj cannot take the map) on Mc rows into `s` and copied through m->dense_src,
 *   - attn densely into a->attn (s->attn takes the Mc-row form where o_proj cannot read the dense rows), lse into a->lse.
 * Of `s` only xn1, qkv, attn, xn2, act are ever used; none of them may be the same buffer as its namesake in `a`.  m->dense_own is not read.
 * vlr_decoder_layer_bwd_src: vlr_decoder_layer_bwd call for call, in the same order, at M = batch * S rows, on such a set.  x_in holds
 * the KEPT rows of the layer's input (the previous layer's a->x_out, or the embedding rows gathered through compact_rows); both norm
 * backwards are the _src forms over src_rows = dense_src; the SwiGLU backward is vlr_gemm_swiglu_bwd_src into dgu [M][2I], a scratch
 * all layers may share, which must not overlap a->gu.  a->gu stays the forward's gate | up.  dx_out, dx_in, `ws` and pos are dense, as
 * for vlr_decoder_layer_bwd, and ws->dqkv holds d qkv [M] afterwards.  Every weight gradient and dx_in equal, bit for bit, those of
 * vlr_decoder_layer_fwd_compact_ex + vlr_layer_acts_expand + vlr_decoder_layer_bwd.
 * Preconditions: no null pointer but key_mask, in the structs too; every src_rows / dense_src entry in [0, Mc); nothing is allocated. */
int vlr_decoder_layer_fwd_compact_keep(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_acts* a,
                                       const vlr_layer_acts* s, const void* x_in, const vlr_row_maps* m, const int* key_mask, int batch,
                                       int S, vlr_stream_t stream);
int vlr_decoder_layer_bwd_src(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_grads* g, int accumulate,
                              const vlr_layer_acts* a, const vlr_layer_bwd_ws* ws, void* dgu, const int* src_rows, const void* x_in,
                              const void* dx_out, void* dx_in, const int* pos, const int* key_mask, int batch, int S,
                              vlr_stream_t stream);
/* 1: every kept row of the row-compact forward over Mc of batch * S rows is computed by the kernel, and in the K order, the dense
 * forward computes it in - the two passes agree bit for bit on the kept rows (16-byte aligned operands assumed).  Host arithmetic
 * only: all four projections take the persistent 256-tile kernel at batch * S and at Mc rows, and the rows the dense residual
 * projections peel (vlr_gemm_peel_rows) lie inside the tail_rows kept last rows.  0 otherwise, and for arguments out of range. */
int vlr_decoder_layer_compact_exact(const vlr_llama_cfg* cfg, int batch, int S, int Mc, int tail_rows);

/* ---- LoRA (peft) adapters on the seven decoder linears (reference: LoraConfig built in utils/auto_load.py:559-571 from
 * LlavaForRL.default_lora_target, Llava/__init__.py:273-286; r/alpha/dropout defaults dpo.py:60-63, scripts/ddpo_llava.sh:24-31).
 * peft semantics: y = base(x) + scale * lora_B(lora_A(dropout(x))), scale = lora_alpha / r, base weights frozen.  The path is
 * un-merged: lora_dropout works and the frozen base weights serve as the reference model (adapter disabled, trl
 * null_ref_context).  Sub-targets of a fused group are stacked: A_*: [n*r][in], B_*: [n*out][r].
 * u [M][7r] (columns qkv | o | gate,up | down) = dropout_t(x) A_t^T, written by the forward and read by the backward.
 * ws_v: scratch [M][3r]; ws_xd: the forward ignores it (ABI v3 stored the seven dropped inputs there: 0.9 GB per layer at the 7B
 * shapes); the backward with dropout > 0 needs ONE scratch [M][max(hidden, inter)] shared by all layers.  Dropout target t of the layer
 * draws its mask from vlr_dropout(seed + t), t = 0..6 in q,k,v,o,gate,up,down order; the mask is applied to x while the skinny GEMMs
 * stage it (vlr_gemm_grouped) and regenerated in the backward - drop(x) is never written. */
typedef struct {
    int r;
    float scale;     /* lora_alpha / r */
    float dropout;   /* 0 in eval mode */
    const void* a_qkv; const void* b_qkv;   /* [3r][H], [3H][r] */
    const void* a_o;   const void* b_o;     /* [r][H],  [H][r]  */
    const void* a_gu;  const void* b_gu;    /* [2r][H], [2I][r] */
    const void* a_down; const void* b_down; /* [r][I],  [H][r]; both NULL: no adapter on the down projection */
    int qkv_targets;  /* 0 or 3: q_proj, k_proj, v_proj adapted separately (a_qkv [3r][H], u_q | u_k | u_v); 1: ONE adapter on the
                       * fused projection (Qwen c_attn: a_qkv [r][H], b_qkv [N][r]) */
    void* mask_bits;  /* ABI v5, dropout > 0 only: vlr_lora_mask_bytes(hidden, inter, M) bytes of THIS layer, or NULL.  The forward draws
                       * the seven packed keep masks into it in both forms of vlr_dropout_bits2 (row-major: target t < 6 at t * M * hidden
                       * / 8, down at 6 * M * hidden / 8; behind them, 64-byte aligned, the K-tile-blocked transposed ones) and the adapter
                       * GEMMs of the forward AND of the backward read them; NULL: every kernel hashes */
} vlr_lora_weights;
long vlr_lora_mask_bytes(int hidden, int inter, int M);
typedef struct {
    void* a_qkv; void* b_qkv; void* a_o; void* b_o; void* a_gu; void* b_gu; void* a_down; void* b_down;
} vlr_lora_grads;
int vlr_decoder_layer_fwd_lora(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_lora_weights* lw,
                               const vlr_layer_acts* a, void* u, void* ws_xd, uint64_t seed, const void* x_in,
                               const int* pos, const int* key_mask, int batch, int S, vlr_stream_t stream);
int vlr_decoder_layer_bwd_lora(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_lora_weights* lw,
                               const vlr_lora_grads* lg, int accumulate, const vlr_layer_acts* a, const void* u,
                               const vlr_layer_bwd_ws* ws, void* ws_v, void* ws_xd, uint64_t seed, const void* x_in,
                               const void* dx_out, void* dx_in, const int* pos, const int* key_mask, int batch, int S,
                               vlr_stream_t stream);
/* The same two passes for a decoder whose linears carry adapters as BASE-MODEL weights on a row subset - PLoRA of InternLM-XComposer2
 * (reference models/InternLMXC2/build_mlp.py:158-203: `res[im_mask] += Plora_B(Plora_A(dropout(x[im_mask])))`, r = 256): rowmask
 * [batch * S] bytes, non-zero = image row (NULL: all rows) - the text rows of u / v are zeroed, so the dense adapter kernels compute
 * exactly the row-restricted update; g != NULL: the base weights train too (full fine-tune: gradients as vlr_decoder_layer_bwd
 * writes them), NULL: frozen.  The dropout mask of target t is vlr_dropout(seed + t) indexed over the FULL [batch * S][in] input. */
int vlr_decoder_layer_fwd_lora_ex(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_lora_weights* lw,
                                  const vlr_layer_acts* a, void* u, void* ws_xd, uint64_t seed, const unsigned char* rowmask,
                                  const void* x_in, const int* pos, const int* key_mask, int batch, int S, vlr_stream_t stream);
int vlr_decoder_layer_bwd_lora_ex(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_grads* g,
                                  const vlr_lora_weights* lw, const vlr_lora_grads* lg, int accumulate, const vlr_layer_acts* a,
                                  const void* u, const vlr_layer_bwd_ws* ws, void* ws_v, void* ws_xd, uint64_t seed,
                                  const unsigned char* rowmask, const void* x_in, const void* dx_out, void* dx_in, const int* pos,
                                  const int* key_mask, int batch, int S, vlr_stream_t stream);
/* ---- ABI v7: TWO adapters per linear - peft LoRA (trainable, every row) stacked on PLoRA (frozen base-model weights, image rows only):
 * what reference scripts/dpo_internlmxc2vl7b.sh trains (--use_lora True over the PLoRA decoder of models/InternLMXC2/build_mlp.py:158-203,
 * LoraConfig from utils/auto_load.py:559-571).  y = W x + s_l B_l A_l drop_l(x) + [image rows] s_p B_p A_p drop_p(x) is ONE adapter segment
 * of rank R = lw->r + pw->r in the K loop of the fused projections: u [M][7R], per sub-target [u_lora (r_l) | u_plora (r_p)], and `bc` holds
 * the groups' row-wise concatenations [B_lora | B_plora] ([n*out][R], vlr_lora_concat_b; rebuilt by the caller when B_lora has moved).  The
 * two adapters draw independent dropout masks (seed_l + t / seed_p + t, their own mask_bits), both indexed over the full [batch*S][in]
 * operand; rowmask applies to the PLoRA half.  Backward: gradients for the LoRA pairs only (lg), input gradients through both; ws_v
 * [M][2R] at least (3R when q, k, v are adapted separately). */
typedef struct { const void* qkv; const void* o; const void* gu; const void* down; } vlr_lora_bcomb;
int vlr_lora_concat_b(const void* b1, int r1, const void* b2, int r2, void* out, long rows, vlr_stream_t stream);
int vlr_decoder_layer_fwd_lora2(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_lora_weights* lw,
                                const vlr_lora_weights* pw, const vlr_lora_bcomb* bc, const vlr_layer_acts* a, void* u,
                                uint64_t seed_l, uint64_t seed_p, const unsigned char* rowmask, const void* x_in, const int* pos,
                                const int* key_mask, int batch, int S, vlr_stream_t stream);
int vlr_decoder_layer_bwd_lora2(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_lora_weights* lw,
                                const vlr_lora_grads* lg, const vlr_lora_weights* pw, const vlr_lora_bcomb* bc, int accumulate,
                                const vlr_layer_acts* a, const void* u, const vlr_layer_bwd_ws* ws, void* ws_v, uint64_t seed_l,
                                uint64_t seed_p, const unsigned char* rowmask, const void* x_in, const void* dx_out, void* dx_in,
                                const int* pos, const int* key_mask, int batch, int S, vlr_stream_t stream);
/* rows of x [M][ld] (first `cols` columns) whose rowmask byte is 0 are zeroed */
int vlr_rows_mask(void* x, int ld, int cols, const unsigned char* rowmask, int M, vlr_stream_t stream);
/* counter-based dropout: out = mask * x * alpha / (1-p)  (add != 0: out += ...); the mask is a pure function of
 * (seed, element index) so the backward regenerates it.  vlr_dropout_mask writes the keep mask as bytes (tests). */
int vlr_dropout(const void* x, void* out, long n, float p, uint64_t seed, float alpha, int add, vlr_stream_t stream);
/* the keep mask of vlr_dropout(seed) over n elements (n % 32 == 0), packed: bit e of byte i = element 8 i + e */
int vlr_dropout_bits(void* bits_u8, long n, float p, uint64_t seed, vlr_stream_t stream);
/* the same mask over a [rows][cols] operand in BOTH packed forms (either pointer may be NULL): row-major as above, and K-tile-blocked
 * transposed - byte ((row / 64) * cols + col) * 8 + (row % 64) / 8, bit e = row + e; vlr_dropout_bits_kt_bytes(rows, cols) bytes, 8-byte
 * aligned - which vlr_gemm_grouped_bits(layout 2, mask_on 3) reads for dA = v^T (mask . x) */
int vlr_dropout_bits2(void* bits_u8, void* bits_kt_u8, int rows, int cols, float p, uint64_t seed, vlr_stream_t stream);
long vlr_dropout_bits_kt_bytes(int rows, int cols);
int vlr_dropout_mask(void* mask_u8, long n, float p, uint64_t seed, vlr_stream_t stream);

/* Kept for callers of earlier ABI versions, when vlr_decoder_layer_bwd could run its weight-gradient GEMMs on a library-owned side
 * stream and this call joined it: every layer pass runs on the caller's stream now, so it does nothing and returns VLR_OK. */
int vlr_layers_join(vlr_stream_t stream);

typedef struct {
    int hidden, mlp, heads, head_dim;
    float ln_eps;
    /* the following default (0) to the CLIP tower of LLaVA; the Qwen-VL tower (QwenVL/visual.py:244-300) sets them */
    int act;            /* MLP activation: 0 / 1 quick_gelu (CLIP), 2 exact GELU (nn.GELU) */
    int head_dim_pad;   /* > head_dim: q|k|v rows and the attention output are laid out with head_dim_pad (128) features per head
                         * (weight rows / columns of the padding are zero) so that head_dim 104 runs on the 128-wide attention kernel;
                         * ws->qkv is [M][3*heads*head_dim_pad], ws->attn [M][heads*head_dim_pad] */
    float attn_scale;   /* softmax scale; 0 = 1/sqrt(head_dim) (of the TRUE head_dim when 0 and head_dim_pad is set) */
} vlr_vit_cfg;
typedef struct {  /* bf16; q|k|v fused [3D][D] + bias [3D] */
    const void* ln1_w; const void* ln1_b; const void* wqkv; const void* bqkv; const void* wo; const void* bo;
    const void* ln2_w; const void* ln2_b; const void* w1; const void* b1; const void* w2; const void* b2;
} vlr_vit_layer_weights;
typedef struct { void* xn; void* qkv; void* attn; void* h; } vlr_vit_ws;   /* [M][D], [M][3D], [M][D], [M][mlp] */
int vlr_vit_layer_fwd(const vlr_vit_cfg* cfg, const vlr_vit_layer_weights* w, const vlr_vit_ws* ws, void* x_inout,
                      int n_img, int T, vlr_stream_t stream);
/* Backward of one CLIP encoder layer for a trainable tower (--freeze_vision_tower False; replaces autograd through transformers
 * CLIPEncoderLayer).  vlr_vit_layer_fwd keeps nothing, so the layer is first recomputed from its input x_in [n_img*T][hidden] into ws
 * (fc1 without the fused activation, so that z exists; h = act(z)), then the chain runs backwards: NN / TN GEMMs, vlr_colsum for the four
 * biases, vlr_layernorm_bwd_res twice, vlr_act_bwd, vlr_attn_bwd (full attention, head_dim 64 or 128).  dx_inout [n_img*T][hidden] holds
 * dL/dx_out on entry and dL/dx_in on return.  grads mirrors the weights (bf16; `accumulate`: +=).  Fixed summation orders, no atomics.
 * A padded head_dim (Qwen-VL's tower) is refused.  ws: xn1, attn, x_mid, xn2, dxn, dattn [M][hidden] (dxn and dattn may be one buffer);
 * qkv, dqkv [M][3*hidden]; z, h, dh [M][mlp]; lse, delta fp32 [n_img][heads][ceil64(T)]; norm_ws vlr_vit_layer_bwd_workspace_bytes. */
typedef struct {
    void* ln1_w; void* ln1_b; void* wqkv; void* bqkv; void* wo; void* bo; void* ln2_w; void* ln2_b; void* w1; void* b1; void* w2; void* b2;
} vlr_vit_layer_grads;
typedef struct {
    void* xn1; void* qkv; void* attn; float* lse; void* x_mid; void* xn2; void* z; void* h;
    void* dh; void* dxn; void* dattn; void* dqkv; float* delta; void* norm_ws;
} vlr_vit_bwd_ws;
int vlr_vit_layer_bwd_workspace_bytes(int hidden, int mlp);
int vlr_vit_layer_bwd(const vlr_vit_cfg* cfg, const vlr_vit_layer_weights* w, const vlr_vit_layer_grads* grads, int accumulate,
                      const void* x_in, const vlr_vit_bwd_ws* ws, void* dx_inout, int n_img, int T, vlr_stream_t stream);

/* ---- decoding with a KV cache (replaces transformers LlamaAttention / LlamaMLP with a DynamicCache during GenerationMixin.generate:
 *      one new token per sequence per step, the K / V of every earlier token kept per layer; reference call site
 *      base/trainer.py:310-360 `model.generate`).  Every kernel below is bound by HBM bandwidth: the weights are read once per step.
 *
 * vlr_gemv_bf16 - skinny GEMM Y [M][N] = X [M][K] . W [N][K]^T for 1 <= M <= 16 (what vlr_gemm_bf16 layout 0 computes; its 128- and
 *   256-row tiles would do 8-256x the work at M = 4).  X, W bf16, fp32 accumulation, K % 8 == 0, any N; X and W 16-byte aligned, W dense
 *   (row stride K).  Split-K partials go to `workspace` (vlr_gemv_workspace_bytes(M, N, K) bytes) and are summed in a fixed order: no
 *   atomics, bit-reproducible.  Epilogue by `mode`:
 *     VLR_GEMV_BF16     Y bf16 [M][ldy] = acc + bias[n] + residual bf16 [M][ldr] (bias / residual NULL = none; Y == residual allowed)
 *     VLR_GEMV_F32      Y fp32 [M][ldy] = acc + bias[n]                                      (lm-head logits)
 *     VLR_GEMV_F32RES   Y fp32 [M][ldy] = acc + residual fp32 [M][ldr]; Y == residual allowed (o_proj / down_proj on vlr_llama_cfg.resid_f32)
 *     VLR_GEMV_QKV_ROPE Y bf16 = acc + bias, then rotate-half RoPE at pos[m] on the first rope_cols columns - the arithmetic of
 *                       vlr_gemm_qkv_rope_bias (rotation of the fp32 accumulators, one rounding)
 *     VLR_GEMV_SWIGLU   N = 2 I (gate | up rows of W): Y bf16 [M][I] = silu(gate) * up - the epilogue of vlr_gemm_swiglu; gate | up is
 *                       not stored
 *   pos / cos_t / sin_t / rope_cols / head_dim / max_pos are read by VLR_GEMV_QKV_ROPE only. */
enum { VLR_GEMV_BF16 = 0, VLR_GEMV_F32 = 1, VLR_GEMV_F32RES = 2, VLR_GEMV_QKV_ROPE = 3, VLR_GEMV_SWIGLU = 4 };
long vlr_gemv_workspace_bytes(int M, int N, int K);
int vlr_gemv_bf16(int mode, const void* X, int ldx, const void* W, void* Y, int ldy, const void* bias, const void* residual, int ldr,
                  const int* pos, const float* cos_t, const float* sin_t, int rope_cols, int head_dim, int max_pos, int M, int N, int K,
                  void* workspace, vlr_stream_t stream);
/* vlr_kv_cache_write - the K / V column blocks k, v of a fused [batch*S][ld] q|k|v buffer (post-RoPE) -> cache columns slot0 ..
 *   slot0 + S - 1 of k_cache, v_cache [batch][kv_heads][cap][head_dim] bf16: an exact copy.  Serves the prefill (S = merged length,
 *   slot0 = 0) and every decode step (S = 1, slot0 = filled length).  Replaces DynamicCache.update's torch.cat. */
int vlr_kv_cache_write(const void* k, const void* v, int ld, void* k_cache, void* v_cache, int batch, int S, int kv_heads,
                       int head_dim, int cap, int slot0, vlr_stream_t stream);
/* vlr_attn_decode_gqa - attention of ONE new query row per sequence against its cache: q [batch][ldq] (head h at columns h*head_dim,
 *   post-RoPE), key_mask [batch][cap] int32 (0 = padded key), the first `len` cache columns (the new token's own included); o bf16
 *   [batch][ldo], head h at h*head_dim.  fp32 softmax with `scale`: the last row of vlr_attn_fwd_gqa (causal) on the same keys.
 *   Split-KV: a workgroup owns (sequence, kv head, key chunk) and the heads / kv_heads query heads of that group (1, 2, 4 or 8); the
 *   partials go to `workspace` (vlr_attn_decode_workspace_bytes(batch, heads, cap) bytes) and a second kernel folds them in chunk
 *   order.  head_dim 128 only (VLR_ERR_ARG otherwise); 1 <= len <= cap. */
long vlr_attn_decode_workspace_bytes(int batch, int heads, int cap);
int vlr_attn_decode_gqa(const void* q, int ldq, const void* k_cache, const void* v_cache, const int* key_mask, void* o, int ldo,
                        void* workspace, int batch, int heads, int kv_heads, int head_dim, int cap, int len, float scale,
                        vlr_stream_t stream);
/* vlr_decoder_layer_decode - one decoder layer (vlr_decoder_layer_fwd_ex's arithmetic) for one new token per sequence:
 *   RMSNorm -> q|k|v + bias + RoPE (vlr_gemv_bf16) -> cache write at column len -> decode attention over len + 1 columns -> o_proj +
 *   residual -> RMSNorm -> gate|up SwiGLU -> down_proj + residual.  x_inout [batch][hidden] is the residual stream (fp32 when
 *   cfg->resid_f32, else bf16), updated in place; pos [batch] the new rows' positions; key_mask [batch][cap] must already mark column
 *   len of every row (the new token).  kv_heads and bqkv are honoured; head_dim 128; len < cap.  Batches above 16 rows run the skinny
 *   GEMMs in 16-row groups - or, with gemv_ws (and the adapter scratch u) sized by the vlr_gemv_wide_* helpers, in 64-row groups
 *   through vlr_gemv_wide_bf16 / _w4 / _lora ("the WIDE skinny GEMM" below): same bits, a quarter of the weight passes.
 *   Scratch: */
typedef struct {
    void* xn;          /* bf16 [batch][hidden] */
    float* rstd;       /* [batch] */
    void* qkv;         /* bf16 [batch][Nq + 2 Nkv] */
    void* attn;        /* bf16 [batch][Nq] */
    void* act;         /* bf16 [batch][inter] */
    void* gemv_ws;     /* >= gemv_ws_bytes: the largest vlr_gemv_workspace_bytes(min(batch, 16), N, K) of the layer's four projections;
                        * batch > 16: the largest vlr_gemv_wide_workspace_bytes(min(batch, 64), N, K) (packed weights:
                        * vlr_gemv_wide_w4_workspace_bytes; with adapters: vlr_gemv_wide_lora_workspace_bytes) selects the 64-row
                        * groups, anything smaller keeps the 16-row groups */
    long gemv_ws_bytes;
    void* attn_ws;     /* >= attn_ws_bytes: vlr_attn_decode_workspace_bytes(batch, heads, cap) */
    long attn_ws_bytes;
} vlr_decode_ws;
int vlr_decoder_layer_decode(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_decode_ws* ws, void* x_inout,
                             const int* pos, void* k_cache, void* v_cache, const int* key_mask, int batch, int cap, int len,
                             vlr_stream_t stream);

/* ---- GPTQ int4 base weights (q_lora: LoRA adapters over a 4-bit base that stays packed in HBM; replaces auto_gptq's QuantLinear
 *      under GPTQConfig(bits=4, disable_exllama=True), reference utils/auto_load.py:520-548).  Checkpoint format "v1" (AutoGPTQ), for a
 *      linear y = x W^T, W [N][K], group size g:
 *        qweight int32 [K/8][N]    nibble j (bits 4j .. 4j+3) of qweight[k8][n] = q[8 k8 + j][n], 0 .. 15
 *        qzeros  int32 [K/g][N/8]  nibble j of qzeros[G][n8] = STORED zero of column 8 n8 + j; the zero used is stored + 1, without
 *                                  wrap-around (stored 15 means 16)
 *        scales  fp16  [K/g][N]
 *        W[n][k] = bf16_rne(float(scales[k/g][n]) * float(q[k][n] - zero[k/g][n]))
 *      The fp32 product is exact (5 x 11 significant bits), so the bf16 rounding is the only one: every entry point below and the
 *      host code (vlrlhf/gptq.py) produce the same bits.  group_size is K itself (the checkpoint's -1) or a multiple of 32 that
 *      divides K; N % 8 == 0; g_idx must be k / g (checked at load time, never read on the device).
 *
 * vlr_gptq_dequant_bf16 - packed -> W bf16 [N][K] dense, K contiguous: what every GEMM here reads.  The engine dequantises ONE decoder
 *   layer into a staging set right before that layer's forward, backward or checkpointed recompute.  qweight and W 16-byte aligned.
 * vlr_gemv_w4 - vlr_gemv_bf16 (same modes, bias, RoPE and residual forms, M <= 16, fixed summation order, bit-reproducible) with W read
 *   packed: an int32 of qweight is one lane's B fragment of v_mfma_f32_16x16x32_bf16, unpacked in registers by the rule above.  The
 *   products are those of vlr_gemv_bf16 on the dequantised matrix; the order in which fp32 partial sums are added differs.  workspace:
 *   vlr_gemv_w4_workspace_bytes(M, N, K) bytes.
 * vlr_decoder_layer_decode_w4 - vlr_decoder_layer_decode with the four projections packed: `w` gives ln1, ln2 and bqkv (its matrix
 *   pointers are not read), `q` the packed q|k|v, o, gate|up and down linears in the engine's fused row order.  ws->gemv_ws must hold
 *   the largest vlr_gemv_w4_workspace_bytes of the four shapes. */
typedef struct { const void* qweight; const void* qzeros; const void* scales; int group_size; } vlr_w4_linear;
typedef struct { vlr_w4_linear qkv, o, gu, down; } vlr_layer_weights_w4;
int vlr_gptq_dequant_bf16(const void* qweight, const void* qzeros, const void* scales, void* W, int K, int N, int group_size,
                          vlr_stream_t stream);
long vlr_gemv_w4_workspace_bytes(int M, int N, int K);
int vlr_gemv_w4(int mode, const void* X, int ldx, const void* qweight, const void* qzeros, const void* scales, int group_size, void* Y,
                int ldy, const void* bias, const void* residual, int ldr, const int* pos, const float* cos_t, const float* sin_t,
                int rope_cols, int head_dim, int max_pos, int M, int N, int K, void* workspace, vlr_stream_t stream);
int vlr_decoder_layer_decode_w4(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_weights_w4* q,
                                const vlr_decode_ws* ws, void* x_inout, const int* pos, void* k_cache, void* v_cache,
                                const int* key_mask, int batch, int cap, int len, vlr_stream_t stream);

/* ---- decoding with LIVE LoRA adapters (peft lora.Linear un-merged during generate: no merged copy of the policy, and the only way to
 *      decode from the cache over a packed GPTQ base, into which nothing can be merged).  Additive entry points: callers of the
 *      adapter-free ones are untouched and vlr_abi_version() does not move.
 *
 * vlr_gemv_bf16_lora / vlr_gemv_w4_lora - vlr_gemv_bf16 / vlr_gemv_w4 (same modes, same argument rules) with the adapter term in the
 *   fp32 accumulator BEFORE the epilogue (bias, RoPE rotation, silu(gate) * up, residual):
 *     acc[m][n] = sum_k X[m][k] W[n][k] + sum_j u[m][t(n) r + j] B[n][j],   u = bf16(scale * X A^T)
 *   A bf16 [targets * r][K] (the sub-targets' lora_A stacked), B bf16 [N][r] in the fused row order, t(n) the sub-target that owns row n:
 *   `outs` (HOST array of `targets` row counts summing to N - q | k | v under grouped-query attention) or NULL for equal blocks of
 *   N / targets rows.  r % 8 == 0 (any such rank), 1 <= targets <= 4; A, B, u 16-byte aligned.
 *   Rounding of u: the fp32 sum x A^T times scale (= lora_alpha / r) in fp32, rounded once to bf16 - the rule of
 *   vlr_decoder_layer_fwd_lora_ex, so a decode step stays within bf16 rounding of the prefill's adapters.
 *   Two steps: the skinny GEMM kernel on A writes split-K partials of x A^T to `u` (vlr_gemv_lora_u_bytes(M, K, targets * r) bytes);
 *   the main launch carries one more K slice whose workgroups fold them in order, round, and write u B^T as the LAST partial slice of
 *   `workspace` (vlr_gemv_lora_workspace_bytes(M, N, K, targets * r) bytes: covers both the bf16 and the packed form).  No atomics,
 *   fixed order, bit-reproducible; B = 0 adds 0.0f last and A = B = NULL runs the adapter-free call: both bit-identical to it.
 * vlr_decoder_layer_decode_lora / _w4_lora - vlr_decoder_layer_decode / _w4 with the adapters of `lora` on q|k|v, o, gate|up and (when
 *   a_down is set) down.  lora->dropout and mask_bits are ignored (decoding is inference).  vlr_decode_ws keeps its layout; gemv_ws must
 *   hold the largest vlr_gemv_lora_workspace_bytes of the four shapes and `lws` gives the u scratch: the largest vlr_gemv_lora_u_bytes
 *   (min(batch, 16), K, targets * r) of the four adapters (K = hidden, except inter for down). */
typedef struct {
    void* u;           /* >= u_bytes */
    long u_bytes;
} vlr_decode_lora_ws;
long vlr_gemv_lora_workspace_bytes(int M, int N, int K, int r_total);
long vlr_gemv_lora_u_bytes(int M, int K, int r_total);
int vlr_gemv_bf16_lora(int mode, const void* X, int ldx, const void* W, void* Y, int ldy, const void* bias, const void* residual, int ldr,
                       const int* pos, const float* cos_t, const float* sin_t, int rope_cols, int head_dim, int max_pos, int M, int N, int K,
                       void* workspace, const void* A, const void* B, int r, int targets, const int* outs, float scale, void* u,
                       vlr_stream_t stream);
int vlr_gemv_w4_lora(int mode, const void* X, int ldx, const void* qweight, const void* qzeros, const void* scales, int group_size, void* Y,
                     int ldy, const void* bias, const void* residual, int ldr, const int* pos, const float* cos_t, const float* sin_t,
                     int rope_cols, int head_dim, int max_pos, int M, int N, int K, void* workspace, const void* A, const void* B, int r,
                     int targets, const int* outs, float scale, void* u, vlr_stream_t stream);
int vlr_decoder_layer_decode_lora(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_lora_weights* lora,
                                  const vlr_decode_ws* ws, const vlr_decode_lora_ws* lws, void* x_inout, const int* pos, void* k_cache,
                                  void* v_cache, const int* key_mask, int batch, int cap, int len, vlr_stream_t stream);
int vlr_decoder_layer_decode_w4_lora(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_weights_w4* q,
                                     const vlr_lora_weights* lora, const vlr_decode_ws* ws, const vlr_decode_lora_ws* lws, void* x_inout,
                                     const int* pos, void* k_cache, void* v_cache, const int* key_mask, int batch, int cap, int len,
                                     vlr_stream_t stream);

/* ---- decoding several samples of one prompt over a SHARED prompt cache (generate(num_return_sequences = n)).  Additive entry points:
 *      vlr_abi_version() does not move.
 *
 * The key side of sample p * fanout + j is two segments:
 *   prompt  k_prompt, v_prompt [prompts][kv_heads][prompt_cap][128] bf16 and prompt_mask [prompts][prompt_cap] int32 (0 = padded key;
 *           prompts are left-padded) - what the prefill writes through vlr_kv_cache_write; the first prompt_len columns are filled.
 *           Shared by the `fanout` samples of prompt p.
 *   tail    k_tail, v_tail [prompts * fanout][kv_heads][tail_cap][128]: the sample's own new tokens.  Columns 0 .. tail_len - 1 are all
 *           attended (no mask); tail_len counts the new token's own column.
 * Columns >= prompt_len of the prompt segment and >= tail_len of a tail are never read.
 *
 * vlr_attn_decode_shared - vlr_attn_decode_gqa for prompts * fanout query rows (q, o as there).  A workgroup owns (prompt, kv head, prompt
 *   key chunk) and all fanout * heads / kv_heads query rows of that prompt, in tiles of 16 (any fanout >= 1): a prompt K/V chunk is read
 *   from HBM once per call, not once per sample.  Both products run on the matrix pipe; the probabilities are rounded to bf16 for P.V
 *   (csrc/decode.hip).  The tails run the kernel of vlr_attn_decode_gqa; one kernel folds prompt chunks, then tail chunks, in order: no
 *   atomics, two calls give the same bits.  heads / kv_heads in {1, 2, 4, 8}; head_dim 128; 1 <= prompt_len <= prompt_cap;
 *   1 <= tail_len <= tail_cap; fanout >= 1.  workspace: vlr_attn_decode_shared_workspace_bytes(...) bytes.
 * vlr_decoder_layer_decode_shared - vlr_decoder_layer_decode (q4 == NULL, lora == NULL), _w4 (q4), _lora (lora, lws) or _w4_lora (both)
 *   at batch = prompts * fanout rows over the shared cache: the new token's K/V column is written to the tails at column tail_len - 1,
 *   attention is vlr_attn_decode_shared, every GEMM call is that of the per-sequence entry points.  ws->attn_ws must hold
 *   vlr_attn_decode_shared_workspace_bytes(prompts, fanout, heads, prompt_cap, tail_cap) bytes. */
typedef struct {
    void* k_prompt; void* v_prompt; const int* prompt_mask;   /* this layer's */
    int prompts, prompt_cap, prompt_len;
    void* k_tail; void* v_tail;
    int fanout, tail_cap, tail_len;                           /* columns attended, the new one included */
} vlr_kv_shared;
long vlr_attn_decode_shared_workspace_bytes(int prompts, int fanout, int heads, int prompt_cap, int tail_cap);
int vlr_attn_decode_shared(const void* q, int ldq, const vlr_kv_shared* kv, void* o, int ldo, void* workspace, int heads, int kv_heads,
                           int head_dim, float scale, vlr_stream_t stream);
int vlr_decoder_layer_decode_shared(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_weights_w4* q4,
                                    const vlr_lora_weights* lora, const vlr_decode_ws* ws, const vlr_decode_lora_ws* lws, void* x_inout,
                                    const int* pos, const vlr_kv_shared* kv, vlr_stream_t stream);

/* ---- the WIDE skinny GEMM: up to 64 rows in ONE pass over the weights (sampling 32 - 64 sequences at once, reference
 *      base/trainer.py:437-442 batch_size=32 and num_return_sequences: the 16-row calls stream every weight ceil(M / 16) times per
 *      token).  Additive entry points: the 16-row ones, their M <= 16 rule and their workspace helpers are untouched and
 *      vlr_abi_version() does not move.
 *
 * vlr_gemv_wide_bf16 / vlr_gemv_wide_bf16_lora - the argument lists and rules of vlr_gemv_bf16 / vlr_gemv_bf16_lora with 1 <= M <= 64.
 *   A lane's W fragments of a k step feed ceil(M / 16) row tiles; grid, K slices, chunk order, the four-wave fold and the partial
 *   layout are those of the 16-row kernel, so every output element is summed in the same order: the result equals, BIT FOR BIT, the
 *   16-row entry point called on rows [0, 16), [16, 32), ... of the same X (pos, residual and Y advanced by the same rows).  M <= 16
 *   launches the 16-row kernels themselves.  Workspace and u scratch: the vlr_gemv_wide_* helpers below (>= the 16-row helpers' values,
 *   equal to them at M <= 16).
 * vlr_gemv_wide_w4 / vlr_gemv_wide_w4_lora - the same for packed int4 weights: the argument lists and rules of vlr_gemv_w4 /
 *   vlr_gemv_w4_lora with 1 <= M <= 64.  A lane's packed words are unpacked ONCE per k step and column tile and the fragment feeds
 *   ceil(M / 16) row tiles, so the unpack - what bounds the 16-row packed kernel - is shared by all rows.  Bit for bit vlr_gemv_w4 /
 *   vlr_gemv_w4_lora on rows [0, 16), [16, 32), ...  Workspace: vlr_gemv_wide_w4_workspace_bytes(M, N, K) (= vlr_gemv_w4_workspace_bytes
 *   at M <= 16, M times its per-row size above).  The adapter form takes vlr_gemv_wide_lora_workspace_bytes and
 *   vlr_gemv_wide_lora_u_bytes, which cover the packed split count as their 16-row namesakes do.
 * vlr_decoder_layer_decode / _w4 / _lora / _w4_lora / _shared take the wide calls in 64-row groups when batch > 16 and
 *   ws->gemv_ws_bytes (with adapters also lws->u_bytes) cover the wide helpers' sizes at min(batch, 64) rows; otherwise they run the
 *   16-row groups as before.  Either way the same bits. */
long vlr_gemv_wide_workspace_bytes(int M, int N, int K);
long vlr_gemv_wide_lora_workspace_bytes(int M, int N, int K, int r_total);
long vlr_gemv_wide_lora_u_bytes(int M, int K, int r_total);
long vlr_gemv_wide_w4_workspace_bytes(int M, int N, int K);
int vlr_gemv_wide_bf16(int mode, const void* X, int ldx, const void* W, void* Y, int ldy, const void* bias, const void* residual, int ldr,
                       const int* pos, const float* cos_t, const float* sin_t, int rope_cols, int head_dim, int max_pos, int M, int N, int K,
                       void* workspace, vlr_stream_t stream);
int vlr_gemv_wide_bf16_lora(int mode, const void* X, int ldx, const void* W, void* Y, int ldy, const void* bias, const void* residual,
                            int ldr, const int* pos, const float* cos_t, const float* sin_t, int rope_cols, int head_dim, int max_pos, int M,
                            int N, int K, void* workspace, const void* A, const void* B, int r, int targets, const int* outs, float scale,
                            void* u, vlr_stream_t stream);
int vlr_gemv_wide_w4(int mode, const void* X, int ldx, const void* qweight, const void* qzeros, const void* scales, int group_size,
                     void* Y, int ldy, const void* bias, const void* residual, int ldr, const int* pos, const float* cos_t,
                     const float* sin_t, int rope_cols, int head_dim, int max_pos, int M, int N, int K, void* workspace,
                     vlr_stream_t stream);
int vlr_gemv_wide_w4_lora(int mode, const void* X, int ldx, const void* qweight, const void* qzeros, const void* scales, int group_size,
                          void* Y, int ldy, const void* bias, const void* residual, int ldr, const int* pos, const float* cos_t,
                          const float* sin_t, int rope_cols, int head_dim, int max_pos, int M, int N, int K, void* workspace,
                          const void* A, const void* B, int r, int targets, const int* outs, float scale, void* u, vlr_stream_t stream);

/* ---- data-parallel gradient exchange on RCCL over xGMI (replaces accelerate MULTI_GPU / torch DDP's NCCL all-reduce:
 *      /root/reference accelerate_config/ddp.yaml:1-14; the reference itself never calls a collective).  One process per
 *      GPU, one communicator per process.  RCCL is dlopen'ed at run time (the copy already mapped into the process,
 *      else librccl.so.1; override with VLR_RCCL_LIB).  vlr_comm_unique_id fills `vlr_comm_unique_id_bytes()` HOST
 *      bytes on rank 0; the launcher carries them to every rank; vlr_comm_init blocks until all `world` ranks called
 *      it.  vlr_allreduce_bucket: in-place SUM over one contiguous slice of the flat gradient buffer, enqueued on
 *      `stream` (dtype 0 = bf16, 1 = fp32); 1/world is folded into the optimizer's gradient scale. */
/* vlr_set_comm_cus(k): the persistent GEMM / attention launches leave k CUs (rounded up to whole XCD octets) to the RCCL kernels
 * that run beside the backward (default: environment VLR_COMM_CUS, else 0); vlr_compute_cus() = what is left for them.
 * vlr_comm_probe: diagnostics only - a streaming copy src -> dst of n bytes on exactly `wgs` workgroups, the stand-in for one RCCL
 * ring kernel in the single-GPU interference bench (tools/comm_interference.py); no communicator involved. */
int vlr_set_comm_cus(int k);
int vlr_compute_cus(void);
int vlr_comm_probe(const void* src, void* dst, long n_bytes, int wgs, vlr_stream_t stream);
int vlr_comm_unique_id_bytes(void);
const char* vlr_comm_library(void);   /* path of the RCCL library in use ("" + vlr_last_error() when none loads) */
int vlr_comm_unique_id(void* id_host);
int vlr_comm_init(const void* id_host, int rank, int world, void** comm_out);
/* (ABI v8) ... with a PER-COMMUNICATOR bound on RCCL's channels (one channel = one workgroup of the ring kernel): ncclCommInitRankConfig
 * with minCTAs / maxCTAs, so that the ring kernels fit the CUs vlr_set_comm_cus reserved without the process-wide NCCL_*_NCHANNELS
 * environment (two communicators of one process may differ: bench.py measures one bucket bounded and unbounded).  max_ctas <= 0 = no
 * bound (vlr_comm_init).  VLR_ERR_HIP when the loaded RCCL has no ncclCommInitRankConfig or rejects the configuration - the caller
 * (vlrlhf/parallel.py NativeComm) then agrees with the other ranks and falls back to vlr_comm_init under the environment bound.
 * vlr_comm_rccl_version: ncclGetVersion of the library in use (major * 10000 + minor * 100 + patch; 0: unknown). */
int vlr_comm_init_cfg(const void* id_host, int rank, int world, int min_ctas, int max_ctas, void** comm_out);
int vlr_comm_has_config(void);      /* (ABI v9) 1: the loaded RCCL exports ncclCommInitRankConfig - agreed on by all ranks before vlr_comm_init_cfg is called */
int vlr_comm_rccl_version(void);
int vlr_comm_destroy(void* comm);
int vlr_allreduce_bucket(void* comm, void* buf, long n, int dtype, vlr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
