// Composed passes: one LLaMA decoder layer forward / backward and one CLIP encoder layer forward, sequenced on a
// single HIP stream from the kernel-level entry points.  Pure host code: no allocation, no synchronisation.
//
// Decoder layer (transformers LlamaDecoderLayer; call site /root/reference src/vlrlhf/models/Llava/__init__.py:232):
//   xn1 = RMSNorm(x) ; qkv = xn1 Wqkv^T ; RoPE(q,k) ; attn = softmax(q k^T / sqrt(d) + causal/pad) v
//   x_mid = x + attn Wo^T ; xn2 = RMSNorm(x_mid) ; gu = xn2 Wgu^T ; act = silu(g) * u ; x_out = x_mid + act Wdown^T
// The backward is the exact adjoint, weight gradients written (or accumulated) straight into the flat bf16 gradient
// buffer views passed in `g` - no autograd graph, no temporaries beyond `ws`.
#include <math.h>

#include "../../include/vlr.h"
#include "common.h"

// (ABI: the backward once ran its weight-gradient GEMMs on a second stream and callers joined it here before reading the gradients;
// every pass is on the caller's stream now, so there is nothing to wait for)
extern "C" int vlr_layers_join(vlr_stream_t stream) {
    (void)stream;
    return VLR_OK;
}

#define CHECK(call)                     \
    do {                                \
        int rc_ = (call);               \
        if (rc_ != VLR_OK) return rc_;  \
    } while (0)

// fp32 residual stream (cfg->resid_f32): x_in / x_mid / x_out are fp32 [M][H]; the norms read them in fp32 and the o_proj / down_proj
// GEMMs add their fp32 accumulators to them without any rounding.  The gradient stream stays bf16.
static int norm_fwd(int f32, const void* x, const void* w, void* y, float* rstd, int M, int H, float eps, hipStream_t st) {
    return f32 ? vlr_rmsnorm_fwd_f32((const float*)x, w, y, rstd, M, H, eps, st) : vlr_rmsnorm_fwd(x, w, y, rstd, M, H, eps, st);
}
// src_rows != NULL: x and rstd are read at src_rows[row] (the kept rows in place, vlr_decoder_layer_bwd_src)
static int norm_bwd(int f32, const void* dy, const void* x, const void* w, const float* rstd, const void* dres, void* dx, void* dw,
                    int acc, void* ws, const int* src_rows, int M, int H, hipStream_t st) {
    if (src_rows)
        return f32 ? vlr_rmsnorm_bwd_f32_src(dy, (const float*)x, w, rstd, dres, dx, dw, acc, ws, src_rows, M, H, st)
                   : vlr_rmsnorm_bwd_src(dy, x, w, rstd, dres, dx, dw, acc, ws, src_rows, M, H, st);
    return f32 ? vlr_rmsnorm_bwd_f32(dy, (const float*)x, w, rstd, dres, dx, dw, acc, ws, M, H, st)
               : vlr_rmsnorm_bwd(dy, x, w, rstd, dres, dx, dw, acc, ws, M, H, st);
}
// y = a W^T + residual (NT), on the bf16 or the fp32 stream
static int proj_res(int f32, const void* a, const void* W, void* y, const void* res, int M, int N, int K, hipStream_t st) {
    return f32 ? vlr_gemm_bf16_f32res(0, a, W, (float*)y, (const float*)res, M, N, K, K, K, N, N, st)
               : vlr_gemm_bf16(0, a, W, y, nullptr, res, M, N, K, K, K, N, N, 0, 0, 0, st);
}

static inline const char* off(const void* p, size_t elems) { return (const char*)p + elems * 2; }
static inline char* off(void* p, size_t elems) { return (char*)p + elems * 2; }

// The shapes of a layer pass over M = batch * S token rows: kvh key / value heads (grouped-query attention), the fused q|k|v row
// [Nq | Nkv | Nkv] = N columns, rf = the fp32 residual stream
struct LayerDims { int H, I, M, kvh, Nq, Nkv, N, rf; };
static LayerDims dims_of(const vlr_llama_cfg* cfg, int M) {
    const int kvh = cfg->kv_heads > 0 ? cfg->kv_heads : cfg->heads;
    const int Nq = cfg->heads * cfg->head_dim, Nkv = kvh * cfg->head_dim;
    return LayerDims{cfg->hidden, cfg->inter, M, kvh, Nq, Nkv, Nq + 2 * Nkv, cfg->resid_f32};
}
static int layer_dims(const char* who, const vlr_llama_cfg* cfg, int batch, int S, LayerDims* L) {
    *L = dims_of(cfg, batch * S);
    VLR_REQUIRE(L->kvh > 0 && cfg->heads % L->kvh == 0, "%s: heads %d is not a multiple of kv_heads %d", who, cfg->heads, L->kvh);
    return VLR_OK;
}
// causal attention over the dense layout: qkv [M][N] holds the q | k | v column blocks (RoPE applied), attn / dattn are [M][Nq]
static int attn_fwd(const vlr_llama_cfg* cfg, const LayerDims& L, const void* qkv, void* attn, float* lse, const int* key_mask, int batch,
                    int S, hipStream_t st) {
    return vlr_attn_fwd_gqa(qkv, off(qkv, L.Nq), off(qkv, (size_t)L.Nq + L.Nkv), L.N, attn, L.Nq, lse, key_mask, batch, S, cfg->heads, L.kvh,
                            cfg->head_dim, 1, 1.0f / sqrtf((float)cfg->head_dim), st);
}
static int attn_bwd(const vlr_llama_cfg* cfg, const LayerDims& L, const void* qkv, const void* attn, const void* dattn, const float* lse,
                    float* delta, const int* key_mask, void* dqkv, int batch, int S, hipStream_t st) {
    return vlr_attn_bwd_gqa(qkv, off(qkv, L.Nq), off(qkv, (size_t)L.Nq + L.Nkv), L.N, attn, dattn, L.Nq, lse, delta, key_mask, dqkv,
                            off(dqkv, L.Nq), off(dqkv, (size_t)L.Nq + L.Nkv), L.N, batch, S, cfg->heads, L.kvh, cfg->head_dim, 1,
                            1.0f / sqrtf((float)cfg->head_dim), st);
}

// keep_for_backward = 0 (no-grad reference / evaluation pass): tensors only the backward reads (gate | up) are not written
extern "C" int vlr_decoder_layer_fwd_ex(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_acts* a,
                                        const void* x_in, const int* pos, const int* key_mask, int batch, int S,
                                        int keep_for_backward, vlr_stream_t st) {
    VLR_REQUIRE(cfg && w && a && x_in && pos, "vlr_decoder_layer_fwd: null argument");
    LayerDims L;
    CHECK(layer_dims("vlr_decoder_layer_fwd", cfg, batch, S, &L));
    const auto [H, I, M, kvh, Nq, Nkv, N, rf] = L;
    CHECK(norm_fwd(rf, x_in, w->ln1, a->xn1, a->rstd1, M, H, cfg->rms_eps, st));
    // q|k|v projection with RoPE applied to the fp32 accumulators in the GEMM epilogue (plain GEMM + rope kernel for the rows /
    // shapes the persistent kernel does not take)
    // (a bias of the fused projection - Qwen c_attn - is added to the accumulators before the rotation)
    CHECK(vlr_gemm_qkv_rope_bias(a->xn1, w->wqkv, w->bqkv, a->qkv, pos, cfg->rope_cos, cfg->rope_sin, M, N, Nq + Nkv, H, H, cfg->head_dim,
                                 cfg->max_pos, st));
    CHECK(attn_fwd(cfg, L, a->qkv, a->attn, a->lse, key_mask, batch, S, st));
    CHECK(proj_res(rf, a->attn, w->wo, a->x_mid, x_in, M, H, Nq, st));
    CHECK(norm_fwd(rf, a->x_mid, w->ln2, a->xn2, a->rstd2, M, H, cfg->rms_eps, st));
    // gate|up projection with act = silu(gate) * up computed in the epilogue
    CHECK(vlr_gemm_swiglu(a->xn2, w->wgu, a->gu, a->act, M, I, H, H, keep_for_backward, st));
    CHECK(proj_res(rf, a->act, w->wdown, a->x_out, a->x_mid, M, H, I, st));
    return VLR_OK;
}
// Row-compact layer: the row-wise operators run on the Mc kept rows of a batch whose other rows
// duplicate a kept one (the shared prompt of a DPO pair: causal attention makes the rejected sequence's prompt rows equal the chosen
// sequence's in every layer).  Attention alone sees the dense [batch * S] layout: the q|k|v epilogue stores a shared row to both of its
// dense rows (output row maps; a row copy through dense_src where the fused kernel does not take the shape or no twin map is given), and
// the attention rows are read back through compact_rows; every other call is the entry point of vlr_decoder_layer_fwd_ex at Mc rows.
int vlr_internal_gemm_res_peel(int f32, const void* a, const void* W, void* y, const void* res, int M, int N, int K, int peel_rows,
                               hipStream_t st);      // gemm.hip: proj_res with the rows of the 128x128 kernel named by the caller
// gemm256p.hip: the kernel a launch would pick, as host arithmetic
int vlr_internal_gemm256p_res_variant(int M, int N, int K, int res_f32);
int vlr_internal_gemm256p_fused_takes(int fuse, int N, int K, int rope_cols);
double vlr_internal_tn_pair_saves(int M0, int N0, int M1, int N1);      // gemm.hip: rounds vlr_gemm_bf16_tn_pair saves over two launches on the compute CUs of the moment
// 1: the fused q|k|v + RoPE and gate|up + SwiGLU kernels take every row of this layer's shapes - what a row map on their A operand needs
static int fused_take_all(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const LayerDims& L) {
    return cfg->head_dim == 128 && (!w->bqkv || !((uintptr_t)w->bqkv & 7)) && vlr_internal_gemm256p_fused_takes(2, L.N, L.H, L.Nq + L.Nkv) &&
           vlr_internal_gemm256p_fused_takes(1, 2 * L.I, L.H, 0);
}
// attn_in_place: o_proj reads the kept rows of attn_dense through compact_rows where the persistent kernel takes the launch and the
// peeled rows are the last dense rows (else, and always with attn_in_place = 0, they are compacted into a->attn first).
// twin != NULL: xn1 / xn2 are written to the DENSE rows of a->xn1 / a->xn2 (and a shared row's dropped copy) by the scatter norms and the
// fused projections read them through compact_rows - the caller has asked fused_take_all
// dst_twin != NULL (the caller has asked fused_take_all): the q|k|v + RoPE epilogue stores a kept row straight to its dense row of
// qkv_dense, and a shared row to its dropped copy's too (output maps compact_rows / dst_twin) - a->qkv is not written and no row copy
// rebuilds the dense layout.  Else: q|k|v on Mc rows into a->qkv, expanded through dense_src.
// act_dense (needs twin and dst_twin): the SwiGLU epilogue stores act to the DENSE rows of a->act the same way and down_proj reads the kept
// rows through compact_rows, as o_proj reads the attention rows - the caller has asked act_in_place
static int layer_fwd_compact(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_acts* a, const void* x_in,
                             const int* pos_compact, const int* dense_src, const int* compact_rows, const int* twin, int attn_in_place,
                             int Mc, int tail_rows, void* qkv_dense, void* attn_dense, const int* key_mask, int batch, int S,
                             int keep_for_backward, vlr_stream_t st, const int* dst_twin = nullptr, int act_dense = 0) {
    VLR_REQUIRE(cfg && w && a && x_in && pos_compact && dense_src && compact_rows && qkv_dense && attn_dense,
                "vlr_decoder_layer_fwd_compact: null argument");
    VLR_REQUIRE(batch > 0 && S > 0 && Mc > 0 && Mc <= batch * S, "vlr_decoder_layer_fwd_compact: %d compact rows of %d x %d dense rows", Mc, batch, S);
    LayerDims L;
    CHECK(layer_dims("vlr_decoder_layer_fwd_compact", cfg, batch, S, &L));
    const auto [H, I, M, kvh, Nq, Nkv, N, rf] = L;
    VLR_REQUIRE(tail_rows >= 0 && tail_rows <= Mc, "vlr_decoder_layer_fwd_compact: %d tail rows of %d compact rows", tail_rows, Mc);
    // the two residual projections give their last tile rows to the 128x128 split-K kernel, which sums in another order than the
    // persistent kernel: the rows the DENSE launch peels are peeled here too (they are the last rows of both layouts when they lie
    // inside the kept tail), no others - each row is computed by the kernel the dense pass computes it in.  A dense peel that reaches
    // into dropped rows cannot be reproduced: the launch then splits as its own row count suggests
    const int dense_peel = vlr_gemm_peel_rows(M, H);
    const int peel_rows = dense_peel <= tail_rows ? dense_peel : -1;
    VLR_REQUIRE(!act_dense || (twin && dst_twin), "vlr_decoder_layer_fwd_compact: act on the dense rows needs both twin maps");
    if (twin) {
        CHECK(rf ? vlr_rmsnorm_fwd_f32_scatter((const float*)x_in, w->ln1, a->xn1, a->rstd1, compact_rows, twin, Mc, H, cfg->rms_eps, st)
                 : vlr_rmsnorm_fwd_scatter(x_in, w->ln1, a->xn1, a->rstd1, compact_rows, twin, Mc, H, cfg->rms_eps, st));
    } else {
        CHECK(norm_fwd(rf, x_in, w->ln1, a->xn1, a->rstd1, Mc, H, cfg->rms_eps, st));
    }
    if (dst_twin) {
        CHECK(vlr_gemm_qkv_rope_bias_dst(a->xn1, twin ? compact_rows : nullptr, w->wqkv, w->bqkv, qkv_dense, compact_rows, dst_twin, nullptr, nullptr,
                                         0, pos_compact, cfg->rope_cos, cfg->rope_sin, Mc, N, Nq + Nkv, H, H, cfg->head_dim, cfg->max_pos, st));
    } else {
        if (twin) {
            CHECK(vlr_gemm_qkv_rope_bias_rows(a->xn1, compact_rows, w->wqkv, w->bqkv, a->qkv, pos_compact, cfg->rope_cos, cfg->rope_sin, Mc, N,
                                              Nq + Nkv, H, H, cfg->head_dim, cfg->max_pos, st));
        } else {
            CHECK(vlr_gemm_qkv_rope_bias(a->xn1, w->wqkv, w->bqkv, a->qkv, pos_compact, cfg->rope_cos, cfg->rope_sin, Mc, N, Nq + Nkv, H, H,
                                         cfg->head_dim, cfg->max_pos, st));
        }
        CHECK(vlr_gather_rows(a->qkv, dense_src, qkv_dense, M, N, st));              // dense row m = compact row dense_src[m]
    }
    CHECK(attn_fwd(cfg, L, qkv_dense, attn_dense, a->lse, key_mask, batch, S, st));
    // o_proj straight from the dense attention rows: the rows the 128x128 kernel gets are the last rows of both layouts (peel_rows >= 0:
    // they lie in the kept tail) and reach it by a plain pointer
    if (attn_in_place && H > 512 && peel_rows >= 0 && peel_rows < Mc && vlr_internal_gemm256p_res_variant(Mc - peel_rows, H, Nq, rf) != 0) {
        CHECK(vlr_gemm_res_rows(rf, attn_dense, compact_rows, w->wo, a->x_mid, x_in, Mc, H, Nq, peel_rows, M - peel_rows, st));
    } else {
        CHECK(vlr_gather_rows(attn_dense, compact_rows, a->attn, Mc, Nq, st));       // compact row j = dense row compact_rows[j]
        CHECK(vlr_internal_gemm_res_peel(rf, a->attn, w->wo, a->x_mid, x_in, Mc, H, Nq, peel_rows, st));
    }
    if (twin) {
        CHECK(rf ? vlr_rmsnorm_fwd_f32_scatter((const float*)a->x_mid, w->ln2, a->xn2, a->rstd2, compact_rows, twin, Mc, H, cfg->rms_eps, st)
                 : vlr_rmsnorm_fwd_scatter(a->x_mid, w->ln2, a->xn2, a->rstd2, compact_rows, twin, Mc, H, cfg->rms_eps, st));
        if (act_dense) {
            CHECK(vlr_gemm_swiglu_dst(a->xn2, compact_rows, w->wgu, a->gu, a->act, compact_rows, dst_twin, nullptr, nullptr, 0, Mc, I, H, H,
                                      keep_for_backward ? 1 : 0, st));
            // down_proj straight from the dense act rows; the peeled rows are the last rows of both layouts (act_in_place)
            return vlr_gemm_res_rows(rf, a->act, compact_rows, w->wdown, a->x_out, a->x_mid, Mc, H, I, peel_rows, M - peel_rows, st);
        }
        CHECK(vlr_gemm_swiglu_rows(a->xn2, compact_rows, w->wgu, a->gu, a->act, Mc, I, H, H, keep_for_backward ? 1 : 0, st));
    } else {
        CHECK(norm_fwd(rf, a->x_mid, w->ln2, a->xn2, a->rstd2, Mc, H, cfg->rms_eps, st));
        CHECK(vlr_gemm_swiglu(a->xn2, w->wgu, a->gu, a->act, Mc, I, H, H, keep_for_backward ? 1 : 0, st));
    }
    CHECK(vlr_internal_gemm_res_peel(rf, a->act, w->wdown, a->x_out, a->x_mid, Mc, H, I, peel_rows, st));
    return VLR_OK;
}
// keep_for_backward = 1 (the policy pass): gate | up is written too, as in vlr_decoder_layer_fwd_ex; what the backward reads holds Mc rows
// - a->attn among them (vlr_decoder_layer_bwd_compact reads it): the attention rows are compacted
extern "C" int vlr_decoder_layer_fwd_compact_ex(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_acts* a,
                                                const void* x_in, const int* pos_compact, const int* dense_src, const int* compact_rows,
                                                int Mc, int tail_rows, void* qkv_dense, void* attn_dense, const int* key_mask, int batch,
                                                int S, int keep_for_backward, vlr_stream_t st) {
    return layer_fwd_compact(cfg, w, a, x_in, pos_compact, dense_src, compact_rows, nullptr, keep_for_backward ? 0 : 1, Mc, tail_rows,
                             qkv_dense, attn_dense, key_mask, batch, S, keep_for_backward, st);
}
// the no-grad pass keeps nothing: o_proj reads the dense attention rows through compact_rows (a->attn is then not written)
extern "C" int vlr_decoder_layer_fwd_compact(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_acts* a,
                                             const void* x_in, const int* pos_compact, const int* dense_src, const int* compact_rows,
                                             int Mc, int tail_rows, void* qkv_dense, void* attn_dense, const int* key_mask, int batch,
                                             int S, vlr_stream_t st) {
    return layer_fwd_compact(cfg, w, a, x_in, pos_compact, dense_src, compact_rows, nullptr, 1, Mc, tail_rows, qkv_dense, attn_dense,
                             key_mask, batch, S, 0, st);
}
// vlr_decoder_layer_fwd_compact_ex with the maps as a struct: where m->twin is given and the fused kernels take the layer's shapes, q|k|v is
// stored straight to qkv_dense by the projection's epilogue (a->qkv is not written); every value is vlr_decoder_layer_fwd_compact_ex's
extern "C" int vlr_decoder_layer_fwd_compact_maps(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_acts* a,
                                                  const void* x_in, const vlr_row_maps* m, void* qkv_dense, void* attn_dense,
                                                  const int* key_mask, int batch, int S, int keep_for_backward, vlr_stream_t st) {
    VLR_REQUIRE(cfg && w && a && x_in && m, "vlr_decoder_layer_fwd_compact_maps: null argument");
    VLR_REQUIRE(m->compact_rows && m->dense_src && m->pos_compact, "vlr_decoder_layer_fwd_compact_maps: null row map");
    LayerDims L;
    CHECK(layer_dims("vlr_decoder_layer_fwd_compact_maps", cfg, batch, S, &L));
    const int* dst_twin = m->twin && fused_take_all(cfg, w, L) ? m->twin : nullptr;
    return layer_fwd_compact(cfg, w, a, x_in, m->pos_compact, m->dense_src, m->compact_rows, nullptr, keep_for_backward ? 0 : 1, m->Mc,
                             m->tail_rows, qkv_dense, attn_dense, key_mask, batch, S, keep_for_backward, st, dst_twin, 0);
}
// What vlr_decoder_layer_fwd_compact_ex left on Mc rows (`c`), copied to the dense layout (`d`, batch * S rows) through dense_src: a
// dropped row takes its twin's values, which ARE its values - the dense backward then runs unchanged on `d` and computes what it
// computes after a dense forward.  q|k|v, attn and lse are not copied: the compact forward was given d->qkv / d->attn as its dense
// scratch and d->lse as its lse.  keep_for_backward = 0 (a checkpointed pass): x_out alone
extern "C" int vlr_layer_acts_expand(const vlr_llama_cfg* cfg, const vlr_layer_acts* c, const vlr_layer_acts* d, const int* dense_src,
                                     int M, int keep_for_backward, vlr_stream_t st) {
    VLR_REQUIRE(cfg && c && d && dense_src && M > 0, "vlr_layer_acts_expand: null argument");
    const int H = cfg->hidden, I = cfg->inter;
    const int Hr = cfg->resid_f32 ? 2 * H : H;       // (fp32 residual rows as 16-bit columns)
    VLR_REQUIRE(H % 8 == 0 && I % 8 == 0, "vlr_layer_acts_expand: hidden %d and inter %d must be multiples of 8", H, I);
    VLR_REQUIRE(c->x_out && d->x_out, "vlr_layer_acts_expand: null x_out");
    CHECK(vlr_gather_rows(c->x_out, dense_src, d->x_out, M, Hr, st));
    if (!keep_for_backward) return VLR_OK;
    VLR_REQUIRE(c->xn1 && c->rstd1 && c->x_mid && c->xn2 && c->rstd2 && c->gu && c->act && d->xn1 && d->rstd1 && d->x_mid && d->xn2 &&
                d->rstd2 && d->gu && d->act, "vlr_layer_acts_expand: null activation pointer");
    CHECK(vlr_gather_rows(c->xn1, dense_src, d->xn1, M, H, st));
    CHECK(vlr_gather_f32(c->rstd1, dense_src, d->rstd1, M, st));
    CHECK(vlr_gather_rows(c->x_mid, dense_src, d->x_mid, M, Hr, st));
    CHECK(vlr_gather_rows(c->xn2, dense_src, d->xn2, M, H, st));
    CHECK(vlr_gather_f32(c->rstd2, dense_src, d->rstd2, M, st));
    CHECK(vlr_gather_rows(c->gu, dense_src, d->gu, M, 2 * I, st));
    CHECK(vlr_gather_rows(c->act, dense_src, d->act, M, I, st));
    return VLR_OK;
}
// vlr_decoder_layer_fwd_compact_ex(keep_for_backward = 1) for a backward that reads the kept rows in place (vlr_decoder_layer_bwd_src):
// what only row-wise consumers read - rstd1, x_mid, rstd2, gate | up, x_out - is written on Mc rows into the layer's own set `a` and
// never copied; the operands of the weight-gradient GEMMs, whose mapped dimension would be K - xn1, xn2, act - exist on the M dense rows
// of `a`.  Where the fused kernels take every row of the layer's shapes (the 7B widths) their producers write them there - the scatter
// norms, and the SwiGLU epilogue through its output maps, with down_proj reading the kept rows through compact_rows - and the q|k|v
// epilogue writes a->qkv densely too: nothing is copied and of `s` only s->attn may be written.  Elsewhere (toy widths) they are written
// on Mc rows into `s` and copied.  attn and lse land densely in `a`, as in the expand route
extern "C" int vlr_decoder_layer_fwd_compact_keep(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_acts* a,
                                                  const vlr_layer_acts* s, const void* x_in, const vlr_row_maps* m, const int* key_mask,
                                                  int batch, int S, vlr_stream_t st) {
    VLR_REQUIRE(cfg && w && a && s && x_in && m, "vlr_decoder_layer_fwd_compact_keep: null argument");
    VLR_REQUIRE(m->compact_rows && m->dense_src && m->pos_compact, "vlr_decoder_layer_fwd_compact_keep: null row map");
    VLR_REQUIRE(a->xn1 && a->rstd1 && a->qkv && a->attn && a->lse && a->x_mid && a->xn2 && a->rstd2 && a->gu && a->act && a->x_out &&
                s->xn1 && s->qkv && s->attn && s->xn2 && s->act, "vlr_decoder_layer_fwd_compact_keep: null activation pointer");
    VLR_REQUIRE(a->xn1 != s->xn1 && a->xn2 != s->xn2 && a->act != s->act && a->qkv != s->qkv && a->attn != s->attn,
                "vlr_decoder_layer_fwd_compact_keep: the scratch set must not alias the layer's set");
    const int H = cfg->hidden, I = cfg->inter, M = batch * S;
    VLR_REQUIRE(H % 8 == 0 && I % 8 == 0, "vlr_decoder_layer_fwd_compact_keep: hidden %d and inter %d must be multiples of 8", H, I);
    LayerDims L;
    CHECK(layer_dims("vlr_decoder_layer_fwd_compact_keep", cfg, batch, S, &L));
    // where the fused projections take every row (the 7B shapes; fused_take_all) the norms write xn1 / xn2 to their dense rows and the
    // projections read them through compact_rows; elsewhere they are written on Mc rows into `s` and copied
    const int dense_xn = m->twin && fused_take_all(cfg, w, L);
    // act on its dense rows: down_proj must take the row map - the persistent kernel for all rows but the dense launch's peeled ones, which
    // then have to be the last rows of both layouts (as for o_proj in layer_fwd_compact)
    const int dense_peel = vlr_gemm_peel_rows(M, H);
    const int act_in_place = dense_xn && H > 512 && dense_peel <= m->tail_rows && dense_peel < m->Mc &&
                             vlr_internal_gemm256p_res_variant(m->Mc - dense_peel, H, I, cfg->resid_f32) != 0;
    const vlr_layer_acts t = {dense_xn ? a->xn1 : s->xn1, a->rstd1, s->qkv, s->attn, a->lse, a->x_mid, dense_xn ? a->xn2 : s->xn2, a->rstd2,
                              a->gu, act_in_place ? a->act : s->act, a->x_out};
    CHECK(layer_fwd_compact(cfg, w, &t, x_in, m->pos_compact, m->dense_src, m->compact_rows, dense_xn ? m->twin : nullptr, 1, m->Mc,
                            m->tail_rows, a->qkv, a->attn, key_mask, batch, S, 1, st, dense_xn ? m->twin : nullptr, act_in_place));
    if (!dense_xn) {
        CHECK(vlr_gather_rows(s->xn1, m->dense_src, a->xn1, M, H, st));
        CHECK(vlr_gather_rows(s->xn2, m->dense_src, a->xn2, M, H, st));
    }
    if (!act_in_place) CHECK(vlr_gather_rows(s->act, m->dense_src, a->act, M, I, st));
    return VLR_OK;
}
extern "C" int vlr_decoder_layer_compact_exact(const vlr_llama_cfg* cfg, int batch, int S, int Mc, int tail_rows) {
    if (!cfg || batch <= 0 || S <= 0) return 0;
    const long Ml = (long)batch * S;
    if (Ml > 0x7fffffffL || Mc <= 0 || Mc > Ml || tail_rows < 0 || tail_rows > Mc) return 0;
    const auto [H, I, M, kvh, Nq, Nkv, N, rf] = dims_of(cfg, (int)Ml);
    if (H <= 0 || I <= 0 || kvh <= 0 || cfg->heads % kvh != 0) return 0;
    // q|k|v + RoPE and gate|up + SwiGLU: the fused kernel takes every row of any row count (its peeled tile rows run the same kernel), or
    // none - then the plain GEMM's route depends on the row count
    if (cfg->head_dim != 128 || !vlr_internal_gemm256p_fused_takes(2, N, H, Nq + Nkv) || !vlr_internal_gemm256p_fused_takes(1, 2 * I, H, 0))
        return 0;
    // o_proj / down_proj: the dense launch peels its last rows to the 128x128 split-K kernel; the compact launch peels the same rows when
    // they are kept (vlr_decoder_layer_fwd_compact_ex), and both main parts must run the same variant of the persistent kernel
    const int peel = vlr_gemm_peel_rows(M, H);
    if (peel > tail_rows || peel >= Mc) return 0;
    if (H <= 512) return 0;          // (the skinny split-K route of the plain GEMM is chosen by the row count)
    const int Ks[2] = {Nq, I};
    for (int K : Ks) {
        const int vd = vlr_internal_gemm256p_res_variant(M - peel, H, K, cfg->resid_f32);
        if (vd == 0 || vd != vlr_internal_gemm256p_res_variant(Mc - peel, H, K, cfg->resid_f32)) return 0;
    }
    return 1;
}
extern "C" int vlr_decoder_layer_fwd(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_acts* a,
                                     const void* x_in, const int* pos, const int* key_mask, int batch, int S,
                                     vlr_stream_t st) {
    return vlr_decoder_layer_fwd_ex(cfg, w, a, x_in, pos, key_mask, batch, S, 1, st);
}

// ---- one decoder layer for one new token per sequence against its KV cache (vlr_decoder_layer_fwd_ex's arithmetic at M = batch rows,
// the key side read from the cache).  The skinny GEMMs take at most 16 rows: larger batches run them in 16-row groups, or (`wide`:
// scratch sized for it) in 64-row groups through the wide entry points - one pass over W per 64 rows, the same bits.
// W: the bf16 matrix, or (q != NULL) the packed int4 linear of a GPTQ base (vlr_gemv_w4)
// ad != NULL with ad->A: the live adapter of the projection (vlr_gemv_*_lora)
struct GemvAdapter { const void* A; const void* B; int r, targets; const int* outs; float scale; void* u; };
static int gemv_rows(int mode, const void* X, int ldx, const void* W, const vlr_w4_linear* q, void* Y, int ldy, size_t ysz, const void* bias,
                     const void* res, int ldr, size_t rsz, const int* pos, const vlr_llama_cfg* cfg, int rope_cols, int M, int N, int K,
                     void* ws, hipStream_t st, const GemvAdapter* ad = nullptr, bool wide = false) {
    const int rows = wide ? 64 : 16;
    for (int m0 = 0; m0 < M; m0 += rows) {
        const int mr = M - m0 < rows ? M - m0 : rows;
        const void* x = (const char*)X + (size_t)m0 * ldx * 2;
        void* y = (char*)Y + (size_t)m0 * ldy * ysz;
        const void* r = res ? (const char*)res + (size_t)m0 * ldr * rsz : nullptr;
        const int* p = pos ? pos + m0 : nullptr;
        if (ad && ad->A && q && rows == 64)
            CHECK(vlr_gemv_wide_w4_lora(mode, x, ldx, q->qweight, q->qzeros, q->scales, q->group_size, y, ldy, bias, r, ldr, p, cfg->rope_cos,
                                        cfg->rope_sin, rope_cols, cfg->head_dim, cfg->max_pos, mr, N, K, ws, ad->A, ad->B, ad->r,
                                        ad->targets, ad->outs, ad->scale, ad->u, st));
        else if (q && rows == 64)
            CHECK(vlr_gemv_wide_w4(mode, x, ldx, q->qweight, q->qzeros, q->scales, q->group_size, y, ldy, bias, r, ldr, p, cfg->rope_cos,
                                   cfg->rope_sin, rope_cols, cfg->head_dim, cfg->max_pos, mr, N, K, ws, st));
        else if (ad && ad->A && q)
            CHECK(vlr_gemv_w4_lora(mode, x, ldx, q->qweight, q->qzeros, q->scales, q->group_size, y, ldy, bias, r, ldr, p, cfg->rope_cos,
                                   cfg->rope_sin, rope_cols, cfg->head_dim, cfg->max_pos, mr, N, K, ws, ad->A, ad->B, ad->r, ad->targets,
                                   ad->outs, ad->scale, ad->u, st));
        else if (ad && ad->A && rows == 64)
            CHECK(vlr_gemv_wide_bf16_lora(mode, x, ldx, W, y, ldy, bias, r, ldr, p, cfg->rope_cos, cfg->rope_sin, rope_cols, cfg->head_dim,
                                          cfg->max_pos, mr, N, K, ws, ad->A, ad->B, ad->r, ad->targets, ad->outs, ad->scale, ad->u, st));
        else if (rows == 64)
            CHECK(vlr_gemv_wide_bf16(mode, x, ldx, W, y, ldy, bias, r, ldr, p, cfg->rope_cos, cfg->rope_sin, rope_cols, cfg->head_dim,
                                     cfg->max_pos, mr, N, K, ws, st));
        else if (ad && ad->A)
            CHECK(vlr_gemv_bf16_lora(mode, x, ldx, W, y, ldy, bias, r, ldr, p, cfg->rope_cos, cfg->rope_sin, rope_cols, cfg->head_dim,
                                     cfg->max_pos, mr, N, K, ws, ad->A, ad->B, ad->r, ad->targets, ad->outs, ad->scale, ad->u, st));
        else if (q)
            CHECK(vlr_gemv_w4(mode, x, ldx, q->qweight, q->qzeros, q->scales, q->group_size, y, ldy, bias, r, ldr, p, cfg->rope_cos,
                              cfg->rope_sin, rope_cols, cfg->head_dim, cfg->max_pos, mr, N, K, ws, st));
        else
            CHECK(vlr_gemv_bf16(mode, x, ldx, W, y, ldy, bias, r, ldr, p, cfg->rope_cos, cfg->rope_sin, rope_cols, cfg->head_dim,
                                cfg->max_pos, mr, N, K, ws, st));
    }
    return VLR_OK;
}
// q4 == NULL: the four projections are the bf16 matrices of `w`; else the packed linears of q4 (w gives the norms and the bias)
// lw != NULL: the live adapters of the layer (lws: their u scratch)
static int layer_decode(const char* fn, const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_weights_w4* q4,
                        const vlr_decode_ws* ws, void* x_inout, const int* pos, void* k_cache, void* v_cache, const int* key_mask,
                        int batch, int cap, int len, hipStream_t st, const vlr_lora_weights* lw = nullptr,
                        const vlr_decode_lora_ws* lws = nullptr, const vlr_kv_shared* sh = nullptr) {
    VLR_REQUIRE(cfg && w && ws && x_inout && pos && (sh || (k_cache && v_cache && key_mask)), "%s: null argument", fn);
    if (sh) {      // the shared prompt cache: batch = prompts * fanout rows, the new column is column tail_len - 1 of the tails
        VLR_REQUIRE(sh->k_prompt && sh->v_prompt && sh->prompt_mask && sh->k_tail && sh->v_tail, "%s: null cache pointer", fn);
        VLR_REQUIRE(sh->prompts >= 1, "%s: prompts %d", fn, sh->prompts);
        VLR_REQUIRE(sh->fanout >= 1, "%s: fanout %d must be at least 1", fn, sh->fanout);
        VLR_REQUIRE(sh->prompt_len >= 1 && sh->prompt_len <= sh->prompt_cap, "%s: prompt_len %d outside 1 .. prompt_cap %d", fn,
                    sh->prompt_len, sh->prompt_cap);
        VLR_REQUIRE(sh->tail_len >= 1 && sh->tail_len <= sh->tail_cap, "%s: tail_len %d outside 1 .. tail_cap %d", fn, sh->tail_len,
                    sh->tail_cap);
        batch = sh->prompts * sh->fanout;
        cap = sh->tail_cap;
        len = sh->tail_len - 1;
        k_cache = sh->k_tail;
        v_cache = sh->v_tail;
    }
    VLR_REQUIRE(ws->xn && ws->rstd && ws->qkv && ws->attn && ws->act && ws->gemv_ws && ws->attn_ws, "%s: null scratch buffer", fn);
    VLR_REQUIRE(cfg->head_dim == 128, "%s: head_dim %d unsupported (the decode kernels take head_dim 128)", fn, cfg->head_dim);
    VLR_REQUIRE(batch >= 1, "%s: batch %d", fn, batch);
    VLR_REQUIRE(len >= 0 && len < cap, "%s: len %d must be below the cache capacity cap %d (the new token is written at column len)", fn,
                len, cap);
    const int H = cfg->hidden, I = cfg->inter;
    const int kvh = cfg->kv_heads > 0 ? cfg->kv_heads : cfg->heads;
    VLR_REQUIRE(cfg->heads % kvh == 0, "%s: heads %d is not a multiple of kv_heads %d", fn, cfg->heads, kvh);
    const int Nq = cfg->heads * cfg->head_dim, Nkv = kvh * cfg->head_dim, N = Nq + 2 * Nkv;
    const int mb = batch < 16 ? batch : 16;
    long (*bytes)(int, int, int) = q4 ? vlr_gemv_w4_workspace_bytes : vlr_gemv_workspace_bytes;
    long need = bytes(mb, N, H);
    const long shapes[3] = {bytes(mb, H, Nq), bytes(mb, 2 * I, H), bytes(mb, H, I)};
    for (long b : shapes) need = b > need ? b : need;
    // the 64-row groups: more than 16 rows, and scratch that covers the wide sizes (else the 16-row groups, as ever)
    const int mw = batch < 64 ? batch : 64;
    bool wide = batch > 16;
    long need_w = 0;
    if (wide) {
        long (*wbytes)(int, int, int) = q4 ? vlr_gemv_wide_w4_workspace_bytes : vlr_gemv_wide_workspace_bytes;
        const long wshapes[4] = {wbytes(mw, N, H), wbytes(mw, H, Nq), wbytes(mw, 2 * I, H), wbytes(mw, H, I)};
        for (long b : wshapes) need_w = b > need_w ? b : need_w;
    }
    GemvAdapter a_qkv{}, a_o{}, a_gu{}, a_down{};
    const int o_qkv[3] = {Nq, Nkv, Nkv};
    if (lw) {
        VLR_REQUIRE(lws && lws->u, "%s: null adapter scratch", fn);
        VLR_REQUIRE(lw->r > 0 && lw->r % 8 == 0, "%s: LoRA rank must be a positive multiple of 8, got %d", fn, lw->r);
        VLR_REQUIRE(lw->a_qkv && lw->b_qkv && lw->a_o && lw->b_o && lw->a_gu && lw->b_gu && (!lw->a_down == !lw->b_down), "%s: null adapter pointer", fn);
        VLR_REQUIRE(lw->qkv_targets == 0 || lw->qkv_targets == 1 || lw->qkv_targets == 3, "%s: qkv_targets must be 1 or 3, got %d", fn, lw->qkv_targets);
        const int r = lw->r, nq = lw->qkv_targets == 1 ? 1 : 3;
        a_qkv = GemvAdapter{lw->a_qkv, lw->b_qkv, r, nq, nq == 1 ? nullptr : o_qkv, lw->scale, lws->u};
        a_o = GemvAdapter{lw->a_o, lw->b_o, r, 1, nullptr, lw->scale, lws->u};
        a_gu = GemvAdapter{lw->a_gu, lw->b_gu, r, 2, nullptr, lw->scale, lws->u};
        a_down = GemvAdapter{lw->a_down, lw->b_down, r, 1, nullptr, lw->scale, lws->u};
        const long lshapes[4] = {vlr_gemv_lora_workspace_bytes(mb, N, H, nq * r), vlr_gemv_lora_workspace_bytes(mb, H, Nq, r),
                                 vlr_gemv_lora_workspace_bytes(mb, 2 * I, H, 2 * r), lw->a_down ? vlr_gemv_lora_workspace_bytes(mb, H, I, r) : 0};
        for (long b : lshapes) need = b > need ? b : need;
        long need_u = 0;
        const long ushapes[4] = {vlr_gemv_lora_u_bytes(mb, H, nq * r), vlr_gemv_lora_u_bytes(mb, Nq, r), vlr_gemv_lora_u_bytes(mb, H, 2 * r),
                                 lw->a_down ? vlr_gemv_lora_u_bytes(mb, I, r) : 0};
        for (long b : ushapes) need_u = b > need_u ? b : need_u;
        VLR_REQUIRE(lws->u_bytes >= need_u, "%s: the adapter scratch u has %ld bytes, %ld needed", fn, lws->u_bytes, need_u);
        if (wide) {
            const long wl[4] = {vlr_gemv_wide_lora_workspace_bytes(mw, N, H, nq * r), vlr_gemv_wide_lora_workspace_bytes(mw, H, Nq, r),
                                vlr_gemv_wide_lora_workspace_bytes(mw, 2 * I, H, 2 * r),
                                lw->a_down ? vlr_gemv_wide_lora_workspace_bytes(mw, H, I, r) : 0};
            for (long b : wl) need_w = b > need_w ? b : need_w;
            long need_wu = 0;
            const long wu[4] = {vlr_gemv_wide_lora_u_bytes(mw, H, nq * r), vlr_gemv_wide_lora_u_bytes(mw, Nq, r),
                                vlr_gemv_wide_lora_u_bytes(mw, H, 2 * r), lw->a_down ? vlr_gemv_wide_lora_u_bytes(mw, I, r) : 0};
            for (long b : wu) need_wu = b > need_wu ? b : need_wu;
            wide = lws->u_bytes >= need_wu;
        }
    }
    wide = wide && ws->gemv_ws_bytes >= need_w;
    VLR_REQUIRE(ws->gemv_ws_bytes >= need, "%s: gemv_ws has %ld bytes, %ld needed", fn, ws->gemv_ws_bytes, need);
    const long need_a = sh ? vlr_attn_decode_shared_workspace_bytes(sh->prompts, sh->fanout, cfg->heads, sh->prompt_cap, sh->tail_cap)
                           : vlr_attn_decode_workspace_bytes(batch, cfg->heads, cap);
    VLR_REQUIRE(ws->attn_ws_bytes >= need_a, "%s: attn_ws has %ld bytes, %ld needed", fn, ws->attn_ws_bytes, need_a);
    const int rf = cfg->resid_f32;
    const size_t xs = rf ? 4 : 2;
    const int mode_res = rf ? VLR_GEMV_F32RES : VLR_GEMV_BF16;
    CHECK(norm_fwd(rf, x_inout, w->ln1, ws->xn, ws->rstd, batch, H, cfg->rms_eps, st));
    CHECK(gemv_rows(VLR_GEMV_QKV_ROPE, ws->xn, H, w->wqkv, q4 ? &q4->qkv : nullptr, ws->qkv, N, 2, w->bqkv, nullptr, 0, 0, pos, cfg, Nq + Nkv,
                    batch, N, H, ws->gemv_ws, st, &a_qkv, wide));
    CHECK(vlr_kv_cache_write(off(ws->qkv, Nq), off(ws->qkv, (size_t)Nq + Nkv), N, k_cache, v_cache, batch, 1, kvh, cfg->head_dim, cap, len, st));
    if (sh)
        CHECK(vlr_attn_decode_shared(ws->qkv, N, sh, ws->attn, Nq, ws->attn_ws, cfg->heads, kvh, cfg->head_dim,
                                     1.0f / sqrtf((float)cfg->head_dim), st));
    else
        CHECK(vlr_attn_decode_gqa(ws->qkv, N, k_cache, v_cache, key_mask, ws->attn, Nq, ws->attn_ws, batch, cfg->heads, kvh, cfg->head_dim,
                                  cap, len + 1, 1.0f / sqrtf((float)cfg->head_dim), st));
    CHECK(gemv_rows(mode_res, ws->attn, Nq, w->wo, q4 ? &q4->o : nullptr, x_inout, H, xs, nullptr, x_inout, H, xs, nullptr, cfg, 0, batch, H,
                    Nq, ws->gemv_ws, st, &a_o, wide));
    CHECK(norm_fwd(rf, x_inout, w->ln2, ws->xn, ws->rstd, batch, H, cfg->rms_eps, st));
    CHECK(gemv_rows(VLR_GEMV_SWIGLU, ws->xn, H, w->wgu, q4 ? &q4->gu : nullptr, ws->act, I, 2, nullptr, nullptr, 0, 0, nullptr, cfg, 0, batch,
                    2 * I, H, ws->gemv_ws, st, &a_gu, wide));
    CHECK(gemv_rows(mode_res, ws->act, I, w->wdown, q4 ? &q4->down : nullptr, x_inout, H, xs, nullptr, x_inout, H, xs, nullptr, cfg, 0, batch,
                    H, I, ws->gemv_ws, st, &a_down, wide));
    return VLR_OK;
}
extern "C" int vlr_decoder_layer_decode(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_decode_ws* ws, void* x_inout,
                                        const int* pos, void* k_cache, void* v_cache, const int* key_mask, int batch, int cap, int len,
                                        vlr_stream_t st) {
    return layer_decode("vlr_decoder_layer_decode", cfg, w, nullptr, ws, x_inout, pos, k_cache, v_cache, key_mask, batch, cap, len, st);
}
extern "C" int vlr_decoder_layer_decode_w4(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_weights_w4* q4,
                                           const vlr_decode_ws* ws, void* x_inout, const int* pos, void* k_cache, void* v_cache,
                                           const int* key_mask, int batch, int cap, int len, vlr_stream_t st) {
    VLR_REQUIRE(q4, "vlr_decoder_layer_decode_w4: null packed weights");
    return layer_decode("vlr_decoder_layer_decode_w4", cfg, w, q4, ws, x_inout, pos, k_cache, v_cache, key_mask, batch, cap, len, st);
}

extern "C" int vlr_decoder_layer_decode_lora(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_lora_weights* lora,
                                             const vlr_decode_ws* ws, const vlr_decode_lora_ws* lws, void* x_inout, const int* pos,
                                             void* k_cache, void* v_cache, const int* key_mask, int batch, int cap, int len, vlr_stream_t st) {
    VLR_REQUIRE(lora, "vlr_decoder_layer_decode_lora: null adapters");
    return layer_decode("vlr_decoder_layer_decode_lora", cfg, w, nullptr, ws, x_inout, pos, k_cache, v_cache, key_mask, batch, cap, len, st, lora,
                        lws);
}
extern "C" int vlr_decoder_layer_decode_w4_lora(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_weights_w4* q4,
                                                const vlr_lora_weights* lora, const vlr_decode_ws* ws, const vlr_decode_lora_ws* lws,
                                                void* x_inout, const int* pos, void* k_cache, void* v_cache, const int* key_mask, int batch,
                                                int cap, int len, vlr_stream_t st) {
    VLR_REQUIRE(q4 && lora, "vlr_decoder_layer_decode_w4_lora: null packed weights or adapters");
    return layer_decode("vlr_decoder_layer_decode_w4_lora", cfg, w, q4, ws, x_inout, pos, k_cache, v_cache, key_mask, batch, cap, len, st, lora,
                        lws);
}
// the four routes above over a shared prompt cache (num_return_sequences): q4 and lora pick the route, kv replaces the per-sequence cache
extern "C" int vlr_decoder_layer_decode_shared(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_weights_w4* q4,
                                               const vlr_lora_weights* lora, const vlr_decode_ws* ws, const vlr_decode_lora_ws* lws,
                                               void* x_inout, const int* pos, const vlr_kv_shared* kv, vlr_stream_t st) {
    VLR_REQUIRE(kv, "vlr_decoder_layer_decode_shared: null cache description");
    return layer_decode("vlr_decoder_layer_decode_shared", cfg, w, q4, ws, x_inout, pos, nullptr, nullptr, nullptr, 0, 0, 0, st, lora, lws, kv);
}

// ---- the backward of one decoder layer: ONE sequence (SwiGLU backward, dW pair, dgrad, norm, dW_o, dgrad, attention backward, RoPE
// transpose, dW_qkv, dgrad, norm) for every driver.  What differs between them is data:
//   g     NULL: the base weights are frozen, no weight gradient is computed
//   ad    NULL: no adapters; else the adapter terms of the four linear groups (below)
//   rows  where the rows the pass reads lie (RowLayout)
// An adapter object answers down() - is the down projection adapted - and add(k, x, dy, lddy, dx, dx_fresh): the adapter terms of
// linear group k (0: q|k|v, 1: o, 2: gate|up, 3: down) with input x and output gradient dy [M][lddy] - its adapter gradients, and its
// input-gradient term added to dx, which holds dy W (dx_fresh = 1: WRITTEN to dx; the caller adds dy W afterwards).  LoraBwd and
// Lora2Bwd (with the adapter passes below) are the two implementations; NoAdapter is the type of an absent one
struct NoAdapter {
    bool down() const { return false; }
    int add(int, const void*, const void*, int, void*, int) const { return VLR_OK; }
};
// all NULL: every tensor on its M = batch * S dense rows.
// src_rows + dgu (after vlr_decoder_layer_fwd_compact_keep): the two norm backwards read x_in / rstd1 and x_mid / rstd2 at src_rows[row],
//   the SwiGLU backward reads gate | up there and writes [d gate | d up] to the dense scratch dgu [M][2I], which the weight-gradient
//   pair and the dgrad read in place of a->gu
// m + d (after vlr_decoder_layer_fwd_compact_ex(keep_for_backward = 1)): every row-wise call at m->Mc rows, the attention backward alone
//   on the dense layout, in the scratch d (include/vlr.h); `pos` is m->pos_compact
// (no driver maps rows under an adapter: the adapter products read their operands densely)
struct RowLayout { const int* src_rows; void* dgu; const vlr_row_maps* m; const vlr_dense_scratch* d; };
template <class Adapter>
static int layer_bwd(const vlr_llama_cfg* cfg, const LayerDims& L, const vlr_layer_weights* w, const vlr_layer_grads* g, int accumulate,
                     const vlr_layer_acts* a, const vlr_layer_bwd_ws* ws, const Adapter* ad, const RowLayout& rows, const void* x_in,
                     const void* dx_out, void* dx_in, const int* pos, const int* key_mask, int batch, int S, hipStream_t st) {
    const auto [H, I, M, kvh, Nq, Nkv, N, rf] = L;
    const vlr_row_maps* m = rows.m;
    const vlr_dense_scratch* d = rows.d;
    const int* src_rows = rows.src_rows;
    const int Mr = m ? m->Mc : M;                           // rows of the row-wise calls
    void* gu = src_rows ? rows.dgu : a->gu;                 // [d gate | d up] once the SwiGLU backward has run
    // ---- MLP
    if (src_rows) {
        CHECK(vlr_gemm_swiglu_bwd_src(dx_out, w->wdown, a->gu, src_rows, gu, ws->dact, Mr, I, H, st));
    } else if (ad && ad->down()) {      // adapter terms of down_proj first, then the dgrad GEMM with the SwiGLU backward in its epilogue
        // and those terms as its addend - no separate pass over [M][2I]
        // history: SLOWER than the three separate kernels in round 3 (38.8 ms against 25.5 + 7.7 per step: the addend is a third 16-byte
        // load stream in an epilogue that already reads gate | up), equal in round 4 after the epilogue staging, 1.7 ms FASTER in round 5
        // (482.3 against 484.1 ms, same box, twice each): the default now - no swiglu_bwd_kernel launch under LoRA
        CHECK(ad->add(3, a->act, dx_out, H, ws->dact, 1));
        CHECK(vlr_gemm_swiglu_bwd_add(dx_out, w->wdown, a->gu, ws->dact, ws->dact, Mr, I, H, st));   // gu now holds [dgate | dup]
    } else {
        CHECK(vlr_gemm_swiglu_bwd(dx_out, w->wdown, a->gu, ws->dact, Mr, I, H, st));   // gu now holds [dgate | dup]; d act is not materialised
    }
    // dW_gate|up and dW_down as ONE persistent launch: 1376 + 688 output tiles are 8.06 rounds of 256 CUs together, 6 + 3 apart
    if (g) CHECK(vlr_gemm_bf16_tn_pair(gu, a->xn2, g->wgu, 2 * I, H, 2 * I, H, H, dx_out, a->act, g->wdown, H, I, H, I, I, Mr, accumulate, st));
    CHECK(vlr_gemm_bf16(1, gu, w->wgu, ws->dxn, nullptr, nullptr, Mr, H, 2 * I, 2 * I, H, H, 0, 0, 0, 0, st));
    if (ad) CHECK(ad->add(2, a->xn2, gu, 2 * I, ws->dxn, 0));
    CHECK(norm_bwd(rf, ws->dxn, a->x_mid, w->ln2, a->rstd2, dx_out, ws->dx_mid, g ? g->ln2 : nullptr, g ? accumulate : 0, ws->norm_ws, src_rows,
                   Mr, H, st));
    // ---- attention
    // dW_o is one round of 256 tiles on its own; together with dW_qkv it would be 768 + 256 = 4 whole rounds of ONE persistent launch
    // (vlr_gemm_bf16_tn_pair below; both operands - dx_mid, attn - stay untouched until the end of this call).  Measured NEUTRAL in round 5
    // (565.9 vs 565.9 ms, same box, twice each) on the whole chip; with CUs left to RCCL (240-CU rounds: 4 + 2 apart, 5 together) it saves a
    // round - so: paired when the joint launch saves at least a quarter round on the CUs the launches have now.  That was measured on the
    // adapter-free layer: under an adapter the two launches stay apart
    const bool pair_o = g && !ad && !accumulate && vlr_internal_tn_pair_saves(N, H, H, Nq) >= 0.25;
    if (g && !pair_o) CHECK(vlr_gemm_bf16(2, ws->dx_mid, a->attn, g->wo, nullptr, nullptr, H, Nq, Mr, H, Nq, Nq, 0, 0, accumulate, 0, st));
    CHECK(vlr_gemm_bf16(1, ws->dx_mid, w->wo, ws->dattn, nullptr, nullptr, Mr, Nq, H, H, Nq, Nq, 0, 0, 0, 0, st));
    if (ad) CHECK(ad->add(1, a->attn, ws->dx_mid, H, ws->dattn, 0));
    if (m) {
        // a shared row's d attn is the sum of both branches' gradients already (downstream of it the two copies were one row): it enters at
        // the chosen copy, the dropped copy gets dO = 0 - there delta = 0 and dS = P (dP - delta) = 0 exactly
        CHECK(vlr_expand_rows_zero(ws->dattn, m->dense_own, d->dattn, M, Nq, st));
        CHECK(vlr_gather_rows(a->qkv, m->dense_src, d->qkv, M, N, st));
        CHECK(vlr_gather_rows(a->attn, m->dense_src, d->attn, M, Nq, st));
        CHECK(attn_bwd(cfg, L, d->qkv, d->attn, d->dattn, a->lse, ws->delta, key_mask, d->dqkv, batch, S, st));
        // the rejected response rows' dK / dV on the prompt keys landed on the dropped rows: added to the chosen twin (fp32, one rounding)
        CHECK(vlr_fold_rows(d->dqkv, m->compact_rows, m->twin, ws->dqkv, Mr, N, st));
    } else {
        CHECK(attn_bwd(cfg, L, a->qkv, a->attn, ws->dattn, a->lse, ws->delta, key_mask, ws->dqkv, batch, S, st));
    }
    // transpose of the rotation on the q and k column blocks ((Nq + Nkv) / head_dim consecutive heads)
    CHECK(vlr_rope_heads(ws->dqkv, pos, cfg->rope_cos, cfg->rope_sin, Mr, cfg->heads + kvh, cfg->head_dim, N, cfg->max_pos, 1, st));
    if (pair_o) CHECK(vlr_gemm_bf16_tn_pair(ws->dqkv, a->xn1, g->wqkv, N, H, N, H, H, ws->dx_mid, a->attn, g->wo, H, Nq, H, Nq, Nq, Mr, 0, st));
    else if (g) CHECK(vlr_gemm_bf16(2, ws->dqkv, a->xn1, g->wqkv, nullptr, nullptr, N, H, Mr, N, H, H, 0, 0, accumulate, 0, st));
    CHECK(vlr_gemm_bf16(1, ws->dqkv, w->wqkv, ws->dxn, nullptr, nullptr, Mr, H, N, N, H, H, 0, 0, 0, 0, st));
    if (ad) CHECK(ad->add(0, a->xn1, ws->dqkv, N, ws->dxn, 0));
    CHECK(norm_bwd(rf, ws->dxn, x_in, w->ln1, a->rstd1, ws->dx_mid, dx_in, g ? g->ln1 : nullptr, g ? accumulate : 0, ws->norm_ws, src_rows, Mr, H,
                   st));
    return VLR_OK;
}
extern "C" int vlr_decoder_layer_bwd(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_grads* g,
                                     int accumulate, const vlr_layer_acts* a, const vlr_layer_bwd_ws* ws,
                                     const void* x_in, const void* dx_out, void* dx_in, const int* pos,
                                     const int* key_mask, int batch, int S, vlr_stream_t st) {
    VLR_REQUIRE(cfg && w && g && a && ws && x_in && dx_out && dx_in && pos, "vlr_decoder_layer_bwd: null argument");
    LayerDims L;
    CHECK(layer_dims("vlr_decoder_layer_bwd", cfg, batch, S, &L));
    return layer_bwd(cfg, L, w, g, accumulate, a, ws, (const NoAdapter*)nullptr, RowLayout{}, x_in, dx_out, dx_in, pos, key_mask, batch, S, st);
}
// vlr_decoder_layer_bwd after vlr_decoder_layer_fwd_compact_keep, call for call, in the same order and at M = batch * S rows
extern "C" int vlr_decoder_layer_bwd_src(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_grads* g, int accumulate,
                                         const vlr_layer_acts* a, const vlr_layer_bwd_ws* ws, void* dgu, const int* src_rows,
                                         const void* x_in, const void* dx_out, void* dx_in, const int* pos, const int* key_mask,
                                         int batch, int S, vlr_stream_t st) {
    VLR_REQUIRE(cfg && w && g && a && ws && dgu && src_rows && x_in && dx_out && dx_in && pos, "vlr_decoder_layer_bwd_src: null argument");
    LayerDims L;
    CHECK(layer_dims("vlr_decoder_layer_bwd_src", cfg, batch, S, &L));
    return layer_bwd(cfg, L, w, g, accumulate, a, ws, (const NoAdapter*)nullptr, RowLayout{src_rows, dgu, nullptr, nullptr}, x_in, dx_out, dx_in,
                     pos, key_mask, batch, S, st);
}
// Backward of vlr_decoder_layer_fwd_compact_ex(keep_for_backward = 1)
extern "C" int vlr_decoder_layer_bwd_compact(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_grads* g, int accumulate,
                                             const vlr_layer_acts* a, const vlr_layer_bwd_ws* ws, const vlr_row_maps* m,
                                             const vlr_dense_scratch* d, const void* x_in, const void* dx_out, void* dx_in,
                                             const int* key_mask, int batch, int S, vlr_stream_t st) {
    VLR_REQUIRE(cfg && w && g && a && ws && m && d && x_in && dx_out && dx_in, "vlr_decoder_layer_bwd_compact: null argument");
    VLR_REQUIRE(m->compact_rows && m->dense_src && m->dense_own && m->twin && m->pos_compact, "vlr_decoder_layer_bwd_compact: null row map");
    VLR_REQUIRE(d->qkv && d->attn && d->dattn && d->dqkv, "vlr_decoder_layer_bwd_compact: null dense scratch");
    VLR_REQUIRE(batch > 0 && S > 0 && m->Mc > 0 && m->Mc <= batch * S, "vlr_decoder_layer_bwd_compact: %d compact rows of %d x %d dense rows",
                m->Mc, batch, S);
    LayerDims L;
    CHECK(layer_dims("vlr_decoder_layer_bwd_compact", cfg, batch, S, &L));
    return layer_bwd(cfg, L, w, g, accumulate, a, ws, (const NoAdapter*)nullptr, RowLayout{nullptr, nullptr, m, d}, x_in, dx_out, dx_in,
                     m->pos_compact, key_mask, batch, S, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// LoRA (peft lora.Linear.forward: result = base(x) + lora_B(lora_A(dropout(x))) * scaling) on the seven decoder linears,
// un-merged so that lora_dropout works and the frozen base weights double as the reference model (adapter disabled).
// One fused linear group = n sub-targets sharing the input x [M][in]; y/dy [M][n*out]; A [n*r][in]; B [n*out][r];
// u = dropout_t(x) A_t^T is kept for the backward ([M][7r] per layer: qkv | o | gate,up | down).
// Dropout target t of a layer uses seed + t (t = 0..6 in q,k,v,o,gate,up,down order).
// ---------------------------------------------------------------------------------------------------------------------
// Group k of a layer (0: q|k|v, 1: o, 2: gate|up, 3: down): n sub-targets from target t0 on, reading `in` features - target t has the
// u block at column t * rank, the dropout seed + t and the packed masks of target t; outs[t]: the output features of sub-target t
struct LoraGroup { int n, in, t0, outs[3]; };
// nq = 1: one adapter over the fused projection (Qwen c_attn); 3: q, k, v separately
static LoraGroup lora_group(int k, int nq, const LayerDims& L) {
    if (k == 0) return nq == 1 ? LoraGroup{1, L.H, 0, {L.N}} : LoraGroup{3, L.H, 0, {L.Nq, L.Nkv, L.Nkv}};
    if (k == 1) return LoraGroup{1, L.H, 3, {L.H}};
    if (k == 2) return LoraGroup{2, L.H, 4, {L.I, L.I}};
    return LoraGroup{1, L.I, 6, {L.H}};
}
static long lora_rowmajor_bytes(int hidden, int inter, int M) { return (((long)M * hidden / 8) * 6 + (long)M * inter / 8 + 63) / 64 * 64; }
// the packed keep masks of target t in lw->mask_bits (NULL without dropout): row-major, and K-tile-blocked transposed
struct LoraMasks { unsigned char* bits; unsigned char* bits_kt; };
static inline LoraMasks lora_masks(const vlr_lora_weights* lw, int t, int M, int H, int I) {
    if (!lw->mask_bits || !(lw->dropout > 0.f)) return LoraMasks{nullptr, nullptr};
    unsigned char* base = (unsigned char*)lw->mask_bits;
    return LoraMasks{base + (size_t)t * ((size_t)M * H / 8), base + lora_rowmajor_bytes(H, I, M) + (size_t)t * (size_t)vlr_dropout_bits_kt_bytes(M, H)};
}
// per-stream device buffer for vlr_rows_tile_list (count + tile indices), grown on demand; NULL: no memory (the dense reductions run)
static int* row_tiles_buf(hipStream_t st, int ints) {
    struct Slot { hipStream_t st; int* p; int cap; };
    static Slot slots[8];
    static int nslots = 0;
    Slot* s = nullptr;
    for (int i = 0; i < nslots; ++i) if (slots[i].st == st) s = &slots[i];
    if (!s) { if (nslots == 8) return nullptr; s = &slots[nslots++]; *s = Slot{st, nullptr, 0}; }
    if (s->cap < ints) {
        if (s->p) { hipStreamSynchronize(st); hipFree(s->p); s->p = nullptr; s->cap = 0; }
        const int cap = ints < 16384 ? 16384 : ints;
        if (hipMalloc((void**)&s->p, (size_t)cap * 4) != hipSuccess) { s->p = nullptr; return nullptr; }
        s->cap = cap;
    }
    return s->p;
}
// 256-row tile flags of a row-restricted adapter (1 = no marked row in the tile) for the adapter-segment GEMMs of a layer pass
// (vlr_gemm_seg_rowskip): per-stream device bytes behind the K-tile list of row_tiles_buf; NULL: no row mask or no memory (M % 256 != 0
// never matters: the last tile is simply partial)
static const unsigned char* seg_skip_flags(hipStream_t st, const unsigned char* rowmask, int M) {
    if (!rowmask) return nullptr;
    const int tiles = (M + 255) / 256;
    int* buf = row_tiles_buf(st, M / 64 + 2 + (tiles + 3) / 4);
    if (!buf) return nullptr;
    unsigned char* flags = (unsigned char*)(buf + M / 64 + 2);
    if (vlr_rows_tile_flags(rowmask, M, 256, flags, st) != VLR_OK) return nullptr;
    return flags;
}

// lora_rows.hip: the streaming row-slab adapter products (mode 0: u = alpha (keep . x) A^T, mode 1: v = dy B); false = shape not taken
bool vlr_lora_rows_try_launch(int mode, int n, const void* X, int ldx, const int* Ks, const void* W, int ldw, void* out, int ldo, int ostride,
                              int M, int r, float alpha, const void* bits, long gbits, int bits_ld, const unsigned char* rowmask, hipStream_t st, bool force = false);

// u_t = s * dropout_t(x) A_t^T for the n sub-targets of a group (the B half rides the K loop of the base GEMM: vlr_gemm_*_lora)
// bits != NULL (vlr_lora_weights::mask_bits): the packed keep masks of the n targets are DRAWN here (target t at bits + t * M * in / 8) and
// read by the staged-operand mask of the grouped launch - and again by the backward (lora_group_bwd)
// ustride (0 = r): elements between the u blocks of consecutive sub-targets - the two-adapter layout [u_lora | u_plora] per sub-target
static int lora_group_a(int n, int r, int in, const void* x, int ldx, const void* A, void* u, int ldu, float scale, float p,
                        uint64_t seed, int M, hipStream_t st, const unsigned char* rowmask = nullptr, unsigned char* bits = nullptr,
                        unsigned char* bits_kt = nullptr, int ustride = 0) {
    if (ustride == 0) ustride = r;
    struct MaskAfter {       // PLoRA: the adapter acts on the image rows only - zero the other rows of u on the way out
        void* u; int ldu, n, r, us, M; const unsigned char* rm; hipStream_t st;
        int run() const {
            if (!rm) return VLR_OK;
            if (us == r) return vlr_rows_mask(u, ldu, n * r, rm, M, st);
            for (int t = 0; t < n; ++t) { const int e = vlr_rows_mask((char*)u + (size_t)t * us * 2, ldu, r, rm, M, st); if (e) return e; }
            return VLR_OK;
        }
    } after = {u, ldu, n, r, ustride, M, rowmask, st};
    if (p > 0.f && bits) {      // row-major masks (the streaming u kernel, the dx kernel) and the K-tile-blocked transposed ones (dA) in one draw per target
        VLR_REQUIRE(ldx == in, "lora: the dropout mask is indexed over [M][in]; x must be dense (ldx %d, in %d)", ldx, in);
        VLR_REQUIRE(((long)M * in) % 32 == 0, "lora: packed dropout masks need M * in %% 32 == 0 (M %d, in %d)", M, in);
        const long tstride = vlr_dropout_bits_kt_bytes(M, in);
        for (int t = 0; t < n; ++t)
            CHECK(vlr_dropout_bits2(bits + (size_t)t * ((long)M * in / 8), bits_kt ? bits_kt + (size_t)t * tstride : nullptr, M, in, p, seed + t, st));
    }
    // the streaming row-slab kernel (lora_rows.hip): x read once per target at HBM rate, the text rows of a row-restricted adapter zeroed on
    // the way out; shapes it does not take (and the hashing form without packed masks) run the grouped tile GEMMs below
    if (p == 0.f || bits) {
        const int Ks[4] = {in, in, in, in};
        if (n <= 4 && vlr_lora_rows_try_launch(0, n, x, ldx, Ks, A, in, u, ldu, ustride, M, r, p > 0.f ? scale / (1.f - p) : scale, p > 0.f ? bits : nullptr,
                                               (long)M * in / 8, in, rowmask, st))
            return vlr_check_launch("lora_rows(u)");
    }
    if (p > 0.f) {
        // ONE grouped launch for the n sub-targets: target t = group t reads the SAME x with its own keep mask (vlr_dropout(seed + t),
        // zeroed while the operand is staged - drop(x) is never written) against its own A_t; 1 / (1 - p) rides in alpha
        VLR_REQUIRE(ldx == in, "lora: the dropout mask is indexed over [M][in]; x must be dense (ldx %d, in %d)", ldx, in);
        const long gstride = (long)M * in / 8;
        if (rowmask) CHECK(vlr_gemm_grouped_bits_rows(0, x, A, u, M, r, in, ldx, in, ldu, n, 0L, (long)r * in, (long)ustride, scale / (1.f - p), 0, 1, seed, p,
                                                      in, bits, gstride, rowmask, st));      // all-text tiles are skipped; `after` zeroes the text rows
        else CHECK(vlr_gemm_grouped_bits(0, x, A, u, M, r, in, ldx, in, ldu, n, 0L, (long)r * in, (long)ustride, scale / (1.f - p), 0, 1, seed, p, in, bits,
                                         gstride, st));
    } else if (ustride == r) {
        CHECK(vlr_gemm_bf16_scaled(0, x, A, u, nullptr, nullptr, M, n * r, in, ldx, in, ldu, 0, 0, 0, 0, scale, st));
    } else {
        CHECK(vlr_gemm_grouped(0, x, A, u, M, r, in, ldx, in, ldu, n, 0L, (long)r * in, (long)ustride, scale, 0, 0, 0, 0.f, 0, st));
    }
    return after.run();
}

// dx [M][in] already holds dy W; adds the adapter path and writes the adapter gradients
// outs[t]: output features of sub-target t (they differ under grouped-query attention: q has heads*hd, k and v kv_heads*hd)
// dx_fresh = 1: dx is WRITTEN (= the adapter term alone; the caller adds dy W afterwards - the fused SwiGLU-backward GEMM of down_proj)
static int lora_group_bwd(int n, int r, int in, const int* outs, const void* x, const void* dy, int lddy, const void* A, const void* B,
                          void* dA, void* dB, const void* u, int ldu, void* v, void* dx, float scale, float p, uint64_t seed,
                          int accumulate, int M, hipStream_t st, int dx_fresh = 0, const unsigned char* rowmask = nullptr,
                          const unsigned char* bits = nullptr, const unsigned char* bits_kt = nullptr, const int* ktl = nullptr) {
    const int nr = n * r;
    const long gstride = (long)M * in / 8;       // bytes between the packed keep masks of the group's targets (the forward drew them)
    size_t ofs[4] = {0, 0, 0, 0};
    bool same = true;
    for (int t = 0; t < n; ++t) { ofs[t + 1] = ofs[t] + (size_t)outs[t]; same = same && outs[t] == outs[0]; }
    // dB_t = dy_t^T (s u_t) and v_t = dy_t B_t: the n sub-targets as the groups of one launch each when their widths agree (multi-head
    // attention; grouped-query k / v are narrower than q: one launch per target then)
    const int ng = same ? 1 : n, gs = same ? n : 1;
    // v_t = dy_t B_t for all targets of the group in ONE pass over dy on the streaming row-slab kernel (lora_rows.hip; unmarked rows of a
    // row-restricted adapter come out zero); else per group on the tile GEMMs
    const bool v_done = n <= 4 && vlr_lora_rows_try_launch(1, n, dy, lddy, outs, B, r, v, nr, r, M, r, 1.f, nullptr, 0L, 0, rowmask, st);
    for (int g = 0; g < ng; ++g) {
        const int out = outs[g];
        // (ktl: PLoRA - u and v are zero on the text rows, the K reductions over the token rows read only the 64-row tiles with an image row)
        if (ktl) CHECK(vlr_gemm_grouped_bits_ktiles(2, off(dy, ofs[g]), off(u, (size_t)g * r), off(dB, ofs[g] * r), out, r, M, lddy, ldu, r, gs, (long)out,
                                                    (long)r, (long)out * r, 1.f, accumulate, 0, 0, 0.f, 0, nullptr, 0L, ktl, st));
        else CHECK(vlr_gemm_grouped(2, off(dy, ofs[g]), off(u, (size_t)g * r), off(dB, ofs[g] * r), out, r, M, lddy, ldu, r, gs, (long)out, (long)r,
                                    (long)out * r, 1.f, accumulate, 0, 0, 0.f, 0, st));                  // u is stored scaled
        if (v_done) continue;
        if (rowmask) CHECK(vlr_gemm_grouped_bits_rows(1, off(dy, ofs[g]), off(B, ofs[g] * r), off(v, (size_t)g * r), M, r, out, lddy, r, nr, gs, (long)out,
                                                      (long)out * r, (long)r, 1.f, 0, 0, 0, 0.f, 0, nullptr, 0L, rowmask, st));
        else CHECK(vlr_gemm_grouped(1, off(dy, ofs[g]), off(B, ofs[g] * r), off(v, (size_t)g * r), M, r, out, lddy, r, nr, gs, (long)out,
                                    (long)out * r, (long)r, 1.f, 0, 0, 0, 0.f, 0, st));
    }
    if (rowmask && !v_done) CHECK(vlr_rows_mask(v, nr, nr, rowmask, M, st));      // PLoRA: no gradient flows through the adapter on the text rows
    if (p > 0.f) {
        // dA_t = s / (1 - p) v_t^T (mask_t . x): the n targets as groups, x masked while it is staged (the mask of the forward, regenerated)
        if (bits_kt && ktl) CHECK(vlr_gemm_grouped_bits_ktiles(2, v, x, dA, r, in, M, nr, in, in, n, (long)r, 0L, (long)r * in, scale / (1.f - p), accumulate, 3,
                                                               seed, p, in, bits_kt, vlr_dropout_bits_kt_bytes(M, in), ktl, st));
        else if (bits_kt) CHECK(vlr_gemm_grouped_bits(2, v, x, dA, r, in, M, nr, in, in, n, (long)r, 0L, (long)r * in, scale / (1.f - p), accumulate, 3, seed, p,
                                                      in, bits_kt, vlr_dropout_bits_kt_bytes(M, in), st));
        else CHECK(vlr_gemm_grouped_bits(2, v, x, dA, r, in, M, nr, in, in, n, (long)r, 0L, (long)r * in, scale / (1.f - p), accumulate, 2, seed, p, in,
                                         bits, gstride, st));
        // dx (+)= s / (1 - p) sum_t mask_t . (v_t A_t): ONE pass over dx for the n targets (vlr_gemm_dropout_acc_multi: the streaming kernel
        // of lora_dx.hip, 222 us for q, k, v at [12792 x 4096], r = 128, against 3 x 90 us one target at a time; tools/lora_gemm_bench.py)
        CHECK(vlr_gemm_dropout_acc_multi_rows(n, v, nr, A, dx, M, in, r, p, seed, scale, dx_fresh ? 0 : 1, bits, gstride, rowmask, st));
    } else {
        CHECK(vlr_gemm_bf16_scaled(2, v, x, dA, nullptr, nullptr, nr, in, M, nr, in, in, 0, 0, accumulate, 0, scale, st));  // dA = s v^T x
        CHECK(vlr_gemm_bf16_scaled(1, v, A, dx, nullptr, nullptr, M, in, nr, nr, in, in, 0, 0, dx_fresh ? 0 : 1, 0, scale, st));     // dx (+)= s v A
    }
    return VLR_OK;
}

extern "C" long vlr_lora_mask_bytes(int hidden, int inter, int M) {
    return lora_rowmajor_bytes(hidden, inter, M) + 6 * vlr_dropout_bits_kt_bytes(M, hidden) + vlr_dropout_bits_kt_bytes(M, inter);
}
static int lora_check(const char* who, const vlr_lora_weights* lw) {
    VLR_REQUIRE(lw->r > 0 && lw->r % 8 == 0, "%s: LoRA rank must be a positive multiple of 8, got %d", who, lw->r);
    VLR_REQUIRE(lw->dropout >= 0.f && lw->dropout < 1.f, "%s: lora_dropout must be in [0,1), got %g", who, (double)lw->dropout);
    VLR_REQUIRE(lw->a_qkv && lw->b_qkv && lw->a_o && lw->b_o && lw->a_gu && lw->b_gu && (!lw->a_down == !lw->b_down), "%s: null adapter pointer", who);
    VLR_REQUIRE(lw->qkv_targets == 0 || lw->qkv_targets == 1 || lw->qkv_targets == 3, "%s: qkv_targets must be 1 or 3, got %d", who, lw->qkv_targets);
    return VLR_OK;
}

// y = x W^T + u B^T + residual (NT; the adapter segment of rank R rides the K loop), on the bf16 or the fp32 stream
static int proj_res_lora(int f32, const void* x, const void* W, void* y, const void* res, int M, int N, int K, const void* u, int ldu,
                         const void* B, int R, hipStream_t st) {
    return f32 ? vlr_gemm_lora_f32res(x, K, W, (float*)y, N, (const float*)res, N, M, N, K, u, ldu, B, R, st)
               : vlr_gemm_lora(x, K, W, y, N, res, N, M, N, K, u, ldu, B, R, st);
}
// ---- the forward of one decoder layer under adapters: ONE sequence - vlr_decoder_layer_fwd_ex's, each of the four fused projections
// with an adapter segment of rank R in its K loop.  The segment is made of one or two "sides" (adapters), each with its own rank, scale,
// dropout, A matrices and packed masks (side.w), seed and row mask (NULL: every row): per sub-target the u block [M][R] holds the sides'
// blocks in order, u is [M][7R].
// B: the B operand [out][R] of each projection - one side: the adapter's own b_*; two: their row-wise concatenation (vlr_lora_bcomb)
// skipf (seg_skip_flags; NULL: none): row tiles whose flag is set run only the first skip_col K elements of every sub-target's segment
struct LoraSide { const vlr_lora_weights* w; uint64_t seed; const unsigned char* rowmask; };
static int layer_fwd_lora(const vlr_llama_cfg* cfg, const LayerDims& L, const vlr_layer_weights* w, const LoraSide* sides, int nsides,
                          const vlr_lora_bcomb& B, const unsigned char* skipf, int skip_col, const vlr_layer_acts* a, void* u,
                          const void* x_in, const int* pos, const int* key_mask, int batch, int S, hipStream_t st) {
    const int H = L.H, I = L.I, M = L.M, Nq = L.Nq, Nkv = L.Nkv, N = L.N, rf = L.rf;
    int R = 0;
    for (int s = 0; s < nsides; ++s) R += sides[s].w->r;
    const int ldu = 7 * R;
    const int nq = sides[0].w->qkv_targets == 1 ? 1 : 3;             // one adapter over the fused projection (Qwen c_attn) or q, k, v separately
    // the segment of group k: every side's u = s * dropout(x) A^T, its block behind the previous side's; then the tile skip of the
    // projection that follows
    auto segment = [&](int k, const void* x) -> int {
        const LoraGroup G = lora_group(k, nq, L);
        size_t c = (size_t)G.t0 * R;
        for (int s = 0; s < nsides; ++s) {
            const vlr_lora_weights* lw = sides[s].w;
            const void* const A[4] = {lw->a_qkv, lw->a_o, lw->a_gu, lw->a_down};
            const LoraMasks mk = lora_masks(lw, G.t0, M, H, I);
            CHECK(lora_group_a(G.n, lw->r, G.in, x, G.in, A[k], off(u, c), ldu, lw->scale, lw->dropout, sides[s].seed + G.t0, M, st, sides[s].rowmask,
                               mk.bits, mk.bits_kt, R));
            c += lw->r;
        }
        return vlr_gemm_seg_rowskip(skipf, skip_col);
    };
    CHECK(norm_fwd(rf, x_in, w->ln1, a->xn1, a->rstd1, M, H, cfg->rms_eps, st));
    CHECK(segment(0, a->xn1));
    CHECK(vlr_gemm_qkv_rope_lora(a->xn1, w->wqkv, w->bqkv, a->qkv, pos, cfg->rope_cos, cfg->rope_sin, M, N, Nq + Nkv, H, H,
                                 cfg->head_dim, cfg->max_pos, u, ldu, B.qkv, R, nq == 1 ? N : Nq, nq == 1 ? 0 : Nkv, st));
    CHECK(attn_fwd(cfg, L, a->qkv, a->attn, a->lse, key_mask, batch, S, st));
    CHECK(segment(1, a->attn));
    CHECK(proj_res_lora(rf, a->attn, w->wo, a->x_mid, x_in, M, H, H, off(u, 3 * (size_t)R), ldu, B.o, R, st));
    CHECK(norm_fwd(rf, a->x_mid, w->ln2, a->xn2, a->rstd2, M, H, cfg->rms_eps, st));
    CHECK(segment(2, a->xn2));
    CHECK(vlr_gemm_swiglu_lora(a->xn2, w->wgu, a->gu, a->act, M, I, H, H, off(u, 4 * (size_t)R), ldu, B.gu, R, st));
    if (sides[0].w->a_down) {
        CHECK(segment(3, a->act));
        CHECK(proj_res_lora(rf, a->act, w->wdown, a->x_out, a->x_mid, M, H, I, off(u, 6 * (size_t)R), ldu, B.down, R, st));
    } else {
        CHECK(proj_res(rf, a->act, w->wdown, a->x_out, a->x_mid, M, H, I, st));
    }
    return VLR_OK;
}

extern "C" int vlr_decoder_layer_fwd_lora(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_lora_weights* lw,
                                          const vlr_layer_acts* a, void* u, void* ws_xd, uint64_t seed, const void* x_in,
                                          const int* pos, const int* key_mask, int batch, int S, vlr_stream_t st) {
    return vlr_decoder_layer_fwd_lora_ex(cfg, w, lw, a, u, ws_xd, seed, nullptr, x_in, pos, key_mask, batch, S, st);
}
// rowmask [batch * S] bytes (NULL: every row): the adapters act on the rows whose byte is non-zero only - PLoRA of InternLM-XComposer2
// (reference models/InternLMXC2/build_mlp.py:158-203: im_mask = the image rows)
// (ws_xd is not read: ABI v3 kept drop(x) of the seven targets there; since v4 the mask is applied while the operand is staged)
extern "C" int vlr_decoder_layer_fwd_lora_ex(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_lora_weights* lw,
                                             const vlr_layer_acts* a, void* u, void* ws_xd, uint64_t seed, const unsigned char* rowmask,
                                             const void* x_in, const int* pos, const int* key_mask, int batch, int S, vlr_stream_t st) {
    VLR_REQUIRE(cfg && w && lw && a && u && x_in && pos, "vlr_decoder_layer_fwd_lora: null argument");
    CHECK(lora_check("vlr_decoder_layer_fwd_lora", lw));
    LayerDims L;
    CHECK(layer_dims("vlr_decoder_layer_fwd_lora", cfg, batch, S, &L));
    VLR_REQUIRE(L.Nq == L.H, "vlr_decoder_layer_fwd_lora: heads*head_dim != hidden");
    // a row-restricted adapter (PLoRA alone): row tiles without a marked row skip the WHOLE segment (u is zero there)
    const unsigned char* skipf = (lw->r % 64 == 0) ? seg_skip_flags(st, rowmask, L.M) : nullptr;
    const LoraSide side = {lw, seed, rowmask};
    return layer_fwd_lora(cfg, L, w, &side, 1, vlr_lora_bcomb{lw->b_qkv, lw->b_o, lw->b_gu, lw->b_down}, skipf, 0, a, u, x_in, pos, key_mask, batch,
                          S, st);
}

// the adapter terms of the backward (layer_bwd) under ONE adapter: lora_group_bwd on group k
struct LoraBwd {
    const vlr_lora_weights* lw; const vlr_lora_grads* lg; const void* u; void* v; uint64_t seed; const unsigned char* rowmask; const int* ktl;
    int accumulate; LayerDims L; hipStream_t st;
    bool down() const { return lw->a_down != nullptr; }
    int add(int k, const void* x, const void* dy, int lddy, void* dx, int dx_fresh) const {
        const int r = lw->r;
        const LoraGroup G = lora_group(k, lw->qkv_targets == 1 ? 1 : 3, L);
        const void* const A[4] = {lw->a_qkv, lw->a_o, lw->a_gu, lw->a_down};
        const void* const B[4] = {lw->b_qkv, lw->b_o, lw->b_gu, lw->b_down};
        void* const dA[4] = {lg->a_qkv, lg->a_o, lg->a_gu, lg->a_down};
        void* const dB[4] = {lg->b_qkv, lg->b_o, lg->b_gu, lg->b_down};
        const LoraMasks mk = lora_masks(lw, G.t0, L.M, L.H, L.I);
        return lora_group_bwd(G.n, r, G.in, G.outs, x, dy, lddy, A[k], B[k], dA[k], dB[k], off(u, (size_t)G.t0 * r), 7 * r, v, dx, lw->scale,
                              lw->dropout, seed + G.t0, accumulate, L.M, st, dx_fresh, rowmask, mk.bits, mk.bits_kt, ktl);
    }
};
extern "C" int vlr_decoder_layer_bwd_lora(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_lora_weights* lw,
                                          const vlr_lora_grads* lg, int accumulate, const vlr_layer_acts* a, const void* u,
                                          const vlr_layer_bwd_ws* ws, void* ws_v, void* ws_xd, uint64_t seed, const void* x_in,
                                          const void* dx_out, void* dx_in, const int* pos, const int* key_mask, int batch,
                                          int S, vlr_stream_t st) {
    return vlr_decoder_layer_bwd_lora_ex(cfg, w, nullptr, lw, lg, accumulate, a, u, ws, ws_v, ws_xd, seed, nullptr, x_in, dx_out, dx_in, pos,
                                         key_mask, batch, S, st);
}
// g != NULL: the base weights are trainable too (their gradients as in vlr_decoder_layer_bwd) - the FULL fine-tune of a decoder whose
// linears carry adapters as base-model weights (InternLM-XComposer2's PLoRA); rowmask and ws_xd as in vlr_decoder_layer_fwd_lora_ex
extern "C" int vlr_decoder_layer_bwd_lora_ex(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_layer_grads* g,
                                             const vlr_lora_weights* lw, const vlr_lora_grads* lg, int accumulate, const vlr_layer_acts* a,
                                             const void* u, const vlr_layer_bwd_ws* ws, void* ws_v, void* ws_xd, uint64_t seed,
                                             const unsigned char* rowmask, const void* x_in, const void* dx_out, void* dx_in, const int* pos,
                                             const int* key_mask, int batch, int S, vlr_stream_t st) {
    VLR_REQUIRE(cfg && w && lw && lg && a && u && ws && ws_v && x_in && dx_out && dx_in && pos, "vlr_decoder_layer_bwd_lora: null argument");
    CHECK(lora_check("vlr_decoder_layer_bwd_lora", lw));
    LayerDims L;
    CHECK(layer_dims("vlr_decoder_layer_bwd_lora", cfg, batch, S, &L));
    VLR_REQUIRE(L.Nq == L.H, "vlr_decoder_layer_bwd_lora: heads*head_dim != hidden");
    const int* ktl = nullptr;         // PLoRA: the 64-row K tiles with an image row, for the adapter-gradient reductions over the token rows
    if (rowmask && L.M % 64 == 0 && lg->a_qkv) {
        int* buf = row_tiles_buf(st, L.M / 64 + 1);
        if (buf) { CHECK(vlr_rows_tile_list(rowmask, L.M, buf, st)); ktl = buf; }
    }
    const LoraBwd ad = {lw, lg, u, ws_v, seed, rowmask, ktl, accumulate, L, st};
    return layer_bwd(cfg, L, w, g, accumulate, a, ws, &ad, RowLayout{}, x_in, dx_out, dx_in, pos, key_mask, batch, S, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// TWO adapters per linear: peft LoRA (trainable, every row) stacked on PLoRA (base-model weights, frozen here, image rows only) - the
// configuration reference scripts/dpo_internlmxc2vl7b.sh ships (--use_lora True over the PLoRA decoder of
// models/InternLMXC2/build_mlp.py:158-203; LoraConfig from utils/auto_load.py:559-571).
//   y = W x + s_l B_l A_l drop_l(x) + [image rows] s_p B_p A_p drop_p(x)  =  [x | u_l | u_p] . [W | B_l | B_p]^T
// i.e. ONE adapter segment of rank R = r_l + r_p in the K loop of the fused projections: per sub-target the u block is [u_lora | u_plora]
// (u [M][7R]) and the B operand is the row-wise concatenation [B_lora | B_plora] (vlr_lora_concat_b, built by the caller once per
// optimizer step: B_plora is frozen, B_lora moves).  Dropout: the two adapters draw independent masks (their own seed and packed-mask
// buffer), both indexed over the full [M][in] operand.  Backward: v = dy . [B_l | B_p] in one grouped product; the LoRA half feeds
// dA_l / dB_l and its input-gradient term, the PLoRA half (text rows zeroed) only its input-gradient term.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lora_concat_b_kernel(const bf16_t* __restrict__ b1, int r1, const bf16_t* __restrict__ b2, int r2,
                                                            bf16_t* __restrict__ out, long rows) {
    const int R = r1 + r2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < rows * R; i += (long)gridDim.x * 256) {
        const long row = i / R;
        const int c = (int)(i % R);
        out[i] = c < r1 ? b1[row * r1 + c] : b2[row * r2 + (c - r1)];
    }
}
extern "C" int vlr_lora_concat_b(const void* b1, int r1, const void* b2, int r2, void* out, long rows, vlr_stream_t st) {
    VLR_REQUIRE(b1 && b2 && out && r1 > 0 && r2 > 0 && rows > 0, "vlr_lora_concat_b: bad arguments");
    long blocks = (rows * (r1 + r2) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(lora_concat_b_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)st, (const bf16_t*)b1, r1, (const bf16_t*)b2, r2,
                       (bf16_t*)out, rows);
    return vlr_check_launch("vlr_lora_concat_b");
}

struct Lora2Side {          // one adapter's view of a group
    int r; float scale, p; uint64_t seed; const void* A; void* dA; void* dB; const unsigned char* bits; const unsigned char* bits_kt;
};
// dx [M][in] already holds dy W.  L: the trainable adapter (dA / dB written), P: the frozen row-masked one (dA = dB = NULL).
// dx_fresh = 1: dx is WRITTEN (the adapter terms alone - the first one, LoRA's, covers every row; the caller adds dy W afterwards)
static int lora2_group_bwd(int n, int in, const int* outs, const void* x, const void* dy, int lddy, const Lora2Side& L, const Lora2Side& P,
                           const void* Bcomb, const void* u, int ldu, void* v, void* dx, int accumulate, int M, const unsigned char* rowmask,
                           hipStream_t st, int dx_fresh = 0) {
    int acc_dx = dx_fresh ? 0 : 1;
    const int R = L.r + P.r, nR = n * R;
    const long gstride = (long)M * in / 8;
    size_t ofs[4] = {0, 0, 0, 0};
    bool same = true;
    for (int t = 0; t < n; ++t) { ofs[t + 1] = ofs[t] + (size_t)outs[t]; same = same && outs[t] == outs[0]; }
    const int ng = same ? 1 : n, gs = same ? n : 1;
    // (v_t = dy_t [B_l | B_p]_t as two launches of the streaming row-slab kernel - LoRA columns on every row, PLoRA columns on the image rows -
    // measured 4.5 ms per step SLOWER than the one grouped tile GEMM over all R columns: dy is read twice; gpurun_out r06_rows_auto)
    for (int g = 0; g < ng; ++g) {
        const int out = outs[g];
        // v_t = dy_t [B_l | B_p]_t  ([M][R] per sub-target, sub-targets R apart)
        CHECK(vlr_gemm_grouped(1, off(dy, ofs[g]), off(Bcomb, ofs[g] * R), off(v, (size_t)g * R), M, R, out, lddy, R, nR, gs, (long)out,
                               (long)out * R, (long)R, 1.f, 0, 0, 0, 0.f, 0, st));
        // dB_l,t = dy_t^T u_l,t   (u is stored scaled; the LoRA block is the first r_l columns of the sub-target's u block)
        CHECK(vlr_gemm_grouped(2, off(dy, ofs[g]), off(u, (size_t)g * R), off(L.dB, ofs[g] * L.r), out, L.r, M, lddy, ldu, L.r, gs, (long)out,
                               (long)R, (long)out * L.r, 1.f, accumulate, 0, 0, 0.f, 0, st));
    }
    if (rowmask)
        for (int t = 0; t < n; ++t) CHECK(vlr_rows_mask(off(v, (size_t)t * R + L.r), nR, P.r, rowmask, M, st));      // no gradient through PLoRA on the text rows
    for (int side = 0; side < 2; ++side) {
        const Lora2Side& a = side == 0 ? L : P;
        const size_t c0 = side == 0 ? 0 : (size_t)L.r;                 // column of this adapter's block inside a sub-target's [R]
        for (int t = 0; t < n; ++t) {
            const void* vt = off(v, (size_t)t * R + c0);
            const void* At = off(a.A, (size_t)t * a.r * in);
            if (a.p > 0.f) {
                const unsigned char* bt = a.bits ? a.bits + (size_t)t * gstride : nullptr;
                if (a.dA) {
                    if (a.bits_kt) CHECK(vlr_gemm_grouped_bits(2, vt, x, off(a.dA, (size_t)t * a.r * in), a.r, in, M, nR, in, in, 1, 0L, 0L, 0L,
                                                               a.scale / (1.f - a.p), accumulate, 3, a.seed + t, a.p, in,
                                                               a.bits_kt + (size_t)t * vlr_dropout_bits_kt_bytes(M, in), 0L, st));
                    else CHECK(vlr_gemm_grouped_bits(2, vt, x, off(a.dA, (size_t)t * a.r * in), a.r, in, M, nR, in, in, 1, 0L, 0L, 0L,
                                                     a.scale / (1.f - a.p), accumulate, 2, a.seed + t, a.p, in, bt, 0L, st));
                }
                CHECK(vlr_gemm_dropout_acc_multi_rows(1, vt, nR, At, dx, M, in, a.r, a.p, a.seed + t, a.scale, acc_dx, bt, gstride, side == 1 ? rowmask : nullptr, st));
            } else {
                if (a.dA) CHECK(vlr_gemm_bf16_scaled(2, vt, x, off(a.dA, (size_t)t * a.r * in), nullptr, nullptr, a.r, in, M, nR, in, in, 0, 0,
                                                     accumulate, 0, a.scale, st));
                CHECK(vlr_gemm_bf16_scaled(1, vt, At, dx, nullptr, nullptr, M, in, a.r, nR, in, in, 0, 0, acc_dx, 0, a.scale, st));
            }
            acc_dx = 1;
        }
    }
    return VLR_OK;
}

static int lora2_check(const char* who, const vlr_lora_weights* lw, const vlr_lora_weights* pw, const vlr_lora_bcomb* bc) {
    CHECK(lora_check(who, lw));
    CHECK(lora_check(who, pw));
    VLR_REQUIRE(bc && bc->qkv && bc->o && bc->gu, "%s: null concatenated B", who);
    VLR_REQUIRE((lw->qkv_targets == 1) == (pw->qkv_targets == 1), "%s: the two adapters must split the qkv projection the same way", who);
    VLR_REQUIRE(!lw->a_down == !pw->a_down && (!lw->a_down || bc->down), "%s: down-projection adapters must be both present or both absent", who);
    return VLR_OK;
}

extern "C" int vlr_decoder_layer_fwd_lora2(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_lora_weights* lw,
                                           const vlr_lora_weights* pw, const vlr_lora_bcomb* bc, const vlr_layer_acts* a, void* u,
                                           uint64_t seed_l, uint64_t seed_p, const unsigned char* rowmask, const void* x_in, const int* pos,
                                           const int* key_mask, int batch, int S, vlr_stream_t st) {
    VLR_REQUIRE(cfg && w && lw && pw && a && u && x_in && pos, "vlr_decoder_layer_fwd_lora2: null argument");
    CHECK(lora2_check("vlr_decoder_layer_fwd_lora2", lw, pw, bc));
    LayerDims L;
    CHECK(layer_dims("vlr_decoder_layer_fwd_lora2", cfg, batch, S, &L));
    VLR_REQUIRE(L.Nq == L.H, "vlr_decoder_layer_fwd_lora2: heads*head_dim != hidden");
    const int rl = lw->r, R = rl + pw->r;
    // row tiles without an image row run only the LoRA part (the first rl of every sub-target's R K elements) of the [B_lora | B_plora]
    // segment: the PLoRA block of u is zero there (45 % of the row tiles at 490 x 490 / max_length 1024)
    const unsigned char* skipf = (rl % 64 == 0 && R % 64 == 0) ? seg_skip_flags(st, rowmask, L.M) : nullptr;
    // LoRA block first, PLoRA block behind it (row-masked)
    const LoraSide sides[2] = {{lw, seed_l, nullptr}, {pw, seed_p, rowmask}};
    return layer_fwd_lora(cfg, L, w, sides, 2, *bc, skipf, rl, a, u, x_in, pos, key_mask, batch, S, st);
}

// the adapter terms of the backward (layer_bwd) under LoRA over PLoRA: lora2_group_bwd on group k - gradients for the LoRA pairs only
struct Lora2Bwd {
    const vlr_lora_weights* lw; const vlr_lora_grads* lg; const vlr_lora_weights* pw; const vlr_lora_bcomb* bc; const void* u; void* v;
    uint64_t seed_l, seed_p; const unsigned char* rowmask; int accumulate; LayerDims L; hipStream_t st;
    bool down() const { return lw->a_down != nullptr; }
    int add(int k, const void* x, const void* dy, int lddy, void* dx, int dx_fresh) const {
        const int R = lw->r + pw->r;
        const LoraGroup G = lora_group(k, lw->qkv_targets == 1 ? 1 : 3, L);
        const void* const Al[4] = {lw->a_qkv, lw->a_o, lw->a_gu, lw->a_down};
        const void* const Ap[4] = {pw->a_qkv, pw->a_o, pw->a_gu, pw->a_down};
        const void* const Bc[4] = {bc->qkv, bc->o, bc->gu, bc->down};
        void* const dA[4] = {lg->a_qkv, lg->a_o, lg->a_gu, lg->a_down};
        void* const dB[4] = {lg->b_qkv, lg->b_o, lg->b_gu, lg->b_down};
        const LoraMasks ml = lora_masks(lw, G.t0, L.M, L.H, L.I), mp = lora_masks(pw, G.t0, L.M, L.H, L.I);
        const Lora2Side Ls = {lw->r, lw->scale, lw->dropout, seed_l + (uint64_t)G.t0, Al[k], dA[k], dB[k], ml.bits, ml.bits_kt};
        const Lora2Side Ps = {pw->r, pw->scale, pw->dropout, seed_p + (uint64_t)G.t0, Ap[k], nullptr, nullptr, mp.bits, mp.bits_kt};
        return lora2_group_bwd(G.n, G.in, G.outs, x, dy, lddy, Ls, Ps, Bc[k], off(u, (size_t)G.t0 * R), 7 * R, v, dx, accumulate, L.M, rowmask, st,
                               dx_fresh);
    }
};
extern "C" int vlr_decoder_layer_bwd_lora2(const vlr_llama_cfg* cfg, const vlr_layer_weights* w, const vlr_lora_weights* lw,
                                           const vlr_lora_grads* lg, const vlr_lora_weights* pw, const vlr_lora_bcomb* bc, int accumulate,
                                           const vlr_layer_acts* a, const void* u, const vlr_layer_bwd_ws* ws, void* ws_v, uint64_t seed_l,
                                           uint64_t seed_p, const unsigned char* rowmask, const void* x_in, const void* dx_out, void* dx_in,
                                           const int* pos, const int* key_mask, int batch, int S, vlr_stream_t st) {
    VLR_REQUIRE(cfg && w && lw && lg && pw && a && u && ws && ws_v && x_in && dx_out && dx_in && pos, "vlr_decoder_layer_bwd_lora2: null argument");
    CHECK(lora2_check("vlr_decoder_layer_bwd_lora2", lw, pw, bc));
    LayerDims L;
    CHECK(layer_dims("vlr_decoder_layer_bwd_lora2", cfg, batch, S, &L));
    VLR_REQUIRE(L.Nq == L.H, "vlr_decoder_layer_bwd_lora2: heads*head_dim != hidden");
    const Lora2Bwd ad = {lw, lg, pw, bc, u, ws_v, seed_l, seed_p, rowmask, accumulate, L, st};
    return layer_bwd(cfg, L, w, nullptr, accumulate, a, ws, &ad, RowLayout{}, x_in, dx_out, dx_in, pos, key_mask, batch, S, st);
}

// CLIP encoder layer (transformers CLIPEncoderLayer, pre-LN, quick_gelu; call site Llava/__init__.py:178), in place on x
extern "C" int vlr_vit_layer_fwd(const vlr_vit_cfg* cfg, const vlr_vit_layer_weights* w, const vlr_vit_ws* ws,
                                 void* x, int n_img, int T, vlr_stream_t st) {
    VLR_REQUIRE(cfg && w && ws && x, "vlr_vit_layer_fwd: null argument");
    const int D = cfg->hidden, F = cfg->mlp, M = n_img * T;
    VLR_REQUIRE(cfg->heads * cfg->head_dim == D, "vlr_vit_layer_fwd: heads*head_dim != hidden");
    const int hdp = cfg->head_dim_pad > cfg->head_dim ? cfg->head_dim_pad : cfg->head_dim;   // per-head width of the q|k|v / attention buffers
    const int A = cfg->heads * hdp;
    const float scale = cfg->attn_scale > 0.f ? cfg->attn_scale : 1.0f / sqrtf((float)cfg->head_dim);
    const int act = cfg->act == 2 ? 2 /*gelu*/ : 1 /*quick_gelu*/;
    CHECK(vlr_layernorm_fwd(x, w->ln1_w, w->ln1_b, ws->xn, M, D, cfg->ln_eps, st));
    CHECK(vlr_gemm_bf16(0, ws->xn, w->wqkv, ws->qkv, w->bqkv, nullptr, M, 3 * A, D, D, D, 3 * A, 0, 0, 0, 0, st));
    CHECK(vlr_attn_fwd(ws->qkv, off(ws->qkv, A), off(ws->qkv, 2 * (size_t)A), 3 * A, ws->attn, A, nullptr, nullptr, n_img, T,
                       cfg->heads, hdp, 0, scale, st));
    CHECK(vlr_gemm_bf16(0, ws->attn, w->wo, x, w->bo, x, M, D, A, A, A, D, D, 0, 0, 0, st));
    CHECK(vlr_layernorm_fwd(x, w->ln2_w, w->ln2_b, ws->xn, M, D, cfg->ln_eps, st));
    CHECK(vlr_gemm_bf16(0, ws->xn, w->w1, ws->h, w->b1, nullptr, M, F, D, D, D, F, 0, act, 0, 0, st));
    CHECK(vlr_gemm_bf16(0, ws->h, w->w2, x, w->b2, x, M, D, F, F, F, D, D, 0, 0, 0, st));
    return VLR_OK;
}

// Backward of one CLIP encoder layer with a trainable tower.  The forward above keeps nothing: the layer is recomputed from its input
// x_in into ws (LN1, q|k|v, attention with lse, out-projection + residual, LN2, fc1 WITHOUT the fused activation so that z exists,
// h = act(z)), then the chain runs backwards on existing kernels.  dx holds dL/dx_out on entry and dL/dx_in on return; the residual
// gradient is carried in it (vlr_layernorm_bwd_res adds the norm's branch in place).  Weight gradients by TN GEMMs, bias gradients by
// vlr_colsum, everything in a fixed order: two calls on the same inputs give the same bits.
extern "C" int vlr_vit_layer_bwd_workspace_bytes(int hidden, int mlp) {
    const int c = 3 * hidden > mlp ? 3 * hidden : mlp;
    const int a = vlr_layernorm_bwd_workspace_bytes(hidden), b = vlr_colsum_workspace_bytes(c);
    return a > b ? a : b;
}
extern "C" int vlr_vit_layer_bwd(const vlr_vit_cfg* cfg, const vlr_vit_layer_weights* w, const vlr_vit_layer_grads* g, int accumulate,
                                 const void* x_in, const vlr_vit_bwd_ws* ws, void* dx, int n_img, int T, vlr_stream_t st) {
    VLR_REQUIRE(cfg && w && g && x_in && ws && dx, "vlr_vit_layer_bwd: null argument");
    VLR_REQUIRE(ws->xn1 && ws->qkv && ws->attn && ws->lse && ws->x_mid && ws->xn2 && ws->z && ws->h && ws->dh && ws->dxn && ws->dattn &&
                ws->dqkv && ws->delta && ws->norm_ws, "vlr_vit_layer_bwd: null workspace member");
    VLR_REQUIRE(g->ln1_w && g->ln1_b && g->wqkv && g->bqkv && g->wo && g->bo && g->ln2_w && g->ln2_b && g->w1 && g->b1 && g->w2 && g->b2,
                "vlr_vit_layer_bwd: null gradient member");
    VLR_REQUIRE(n_img > 0 && T > 0, "vlr_vit_layer_bwd: bad shape n_img=%d T=%d", n_img, T);
    const int D = cfg->hidden, F = cfg->mlp, M = n_img * T;
    VLR_REQUIRE(cfg->heads * cfg->head_dim == D, "vlr_vit_layer_bwd: heads*head_dim != hidden");
    VLR_REQUIRE(cfg->head_dim_pad <= cfg->head_dim, "vlr_vit_layer_bwd: a padded head_dim (%d -> %d) has no backward", cfg->head_dim,
                cfg->head_dim_pad);
    const float scale = cfg->attn_scale > 0.f ? cfg->attn_scale : 1.0f / sqrtf((float)cfg->head_dim);
    const int act = cfg->act == 2 ? 2 /*gelu*/ : 1 /*quick_gelu*/;
    const int acc = accumulate ? 1 : 0;
    // ---- the layer again, from x_in
    CHECK(vlr_layernorm_fwd(x_in, w->ln1_w, w->ln1_b, ws->xn1, M, D, cfg->ln_eps, st));
    CHECK(vlr_gemm_bf16(0, ws->xn1, w->wqkv, ws->qkv, w->bqkv, nullptr, M, 3 * D, D, D, D, 3 * D, 0, 0, 0, 0, st));
    CHECK(vlr_attn_fwd(ws->qkv, off(ws->qkv, D), off(ws->qkv, 2 * (size_t)D), 3 * D, ws->attn, D, ws->lse, nullptr, n_img, T, cfg->heads,
                       cfg->head_dim, 0, scale, st));
    CHECK(vlr_gemm_bf16(0, ws->attn, w->wo, ws->x_mid, w->bo, x_in, M, D, D, D, D, D, D, 0, 0, 0, st));
    CHECK(vlr_layernorm_fwd(ws->x_mid, w->ln2_w, w->ln2_b, ws->xn2, M, D, cfg->ln_eps, st));
    CHECK(vlr_gemm_bf16(0, ws->xn2, w->w1, ws->z, w->b1, nullptr, M, F, D, D, D, F, 0, 0, 0, 0, st));
    CHECK(vlr_act_fwd(ws->z, ws->h, (long)M * F, act, st));
    // ---- fc2: x_out = x_mid + h W2^T + b2
    CHECK(vlr_gemm_bf16(2, dx, ws->h, g->w2, nullptr, nullptr, D, F, M, D, F, F, 0, 0, acc, 0, st));
    CHECK(vlr_colsum(dx, M, D, D, g->b2, acc, ws->norm_ws, st));
    CHECK(vlr_gemm_bf16(1, dx, w->w2, ws->dh, nullptr, nullptr, M, F, D, D, F, F, 0, 0, 0, 0, st));
    CHECK(vlr_act_bwd(ws->z, ws->dh, ws->dh, (long)M * F, act, st));                                  // dh <- dz
    // ---- fc1: z = xn2 W1^T + b1
    CHECK(vlr_gemm_bf16(2, ws->dh, ws->xn2, g->w1, nullptr, nullptr, F, D, M, F, D, D, 0, 0, acc, 0, st));
    CHECK(vlr_colsum(ws->dh, M, F, F, g->b1, acc, ws->norm_ws, st));
    CHECK(vlr_gemm_bf16(1, ws->dh, w->w1, ws->dxn, nullptr, nullptr, M, D, F, F, D, D, 0, 0, 0, 0, st));
    CHECK(vlr_layernorm_bwd_res(ws->dxn, ws->x_mid, w->ln2_w, cfg->ln_eps, dx, dx, g->ln2_w, g->ln2_b, acc, ws->norm_ws, M, D, st));   // dx <- d x_mid
    // ---- out-projection: x_mid = x_in + attn Wo^T + bo
    CHECK(vlr_gemm_bf16(2, dx, ws->attn, g->wo, nullptr, nullptr, D, D, M, D, D, D, 0, 0, acc, 0, st));
    CHECK(vlr_colsum(dx, M, D, D, g->bo, acc, ws->norm_ws, st));
    CHECK(vlr_gemm_bf16(1, dx, w->wo, ws->dattn, nullptr, nullptr, M, D, D, D, D, D, 0, 0, 0, 0, st));
    CHECK(vlr_attn_bwd(ws->qkv, off(ws->qkv, D), off(ws->qkv, 2 * (size_t)D), 3 * D, ws->attn, ws->dattn, D, ws->lse, ws->delta, nullptr,
                       ws->dqkv, off(ws->dqkv, D), off(ws->dqkv, 2 * (size_t)D), 3 * D, n_img, T, cfg->heads, cfg->head_dim, 0, scale, st));
    // ---- q|k|v: qkv = xn1 Wqkv^T + bqkv
    CHECK(vlr_gemm_bf16(2, ws->dqkv, ws->xn1, g->wqkv, nullptr, nullptr, 3 * D, D, M, 3 * D, D, D, 0, 0, acc, 0, st));
    CHECK(vlr_colsum(ws->dqkv, M, 3 * D, 3 * D, g->bqkv, acc, ws->norm_ws, st));
    CHECK(vlr_gemm_bf16(1, ws->dqkv, w->wqkv, ws->dxn, nullptr, nullptr, M, D, 3 * D, 3 * D, D, D, 0, 0, 0, 0, st));
    CHECK(vlr_layernorm_bwd_res(ws->dxn, x_in, w->ln1_w, cfg->ln_eps, dx, dx, g->ln1_w, g->ln1_b, acc, ws->norm_ws, M, D, st));       // dx <- d x_in
    return VLR_OK;
}
