"""InternLM-XComposer2 on the MI355X engine (reference /root/reference/src/vlrlhf/models/InternLMXC2/).

What is shared with LLaVA: the CLIP tower (here its LAST hidden state, 35 x 35 patches at 490 px), the mlp2x_gelu projector (frozen
together with the tower, __init__.py:252-255), the <ImageHere> expansion (= the LLaVA merge kernels), grouped-query attention.
What is not:
  * the fused `wqkv` rows are re-ordered from the checkpoint's per-K/V-head layout to q | k | v blocks at load time (engine.ParamLayout);
  * rotary positions are the index in the merged sequence (the vendored apply_rotary_pos_emb ignores position_ids);
  * every decoder linear carries a PLoRA pair that acts on the IMAGE rows only: y[img] += Plora_B(Plora_A(dropout(x[img]))) (build_mlp.py
    :158-203).  They are base-model weights - trained by a full fine-tune, frozen but ACTIVE (reference pass included) under peft LoRA,
    which the shipped script stacks on top of the same five linears.
Every pass runs on the library's layer calls, with the adapters as segments in the K loop of the fused projections (qkv + RoPE,
SwiGLU, residual) and the image rows as the PLoRA row mask, on the fp32 residual stream:
  * full fine-tune and reference pass: `vlr_decoder_layer_fwd_lora_ex` / `bwd_lora_ex` with the PLoRA pairs as the adapters (base and
    PLoRA gradients);
  * peft LoRA over the frozen PLoRA decoder: `vlr_decoder_layer_fwd_lora2` / `bwd_lora2`, two adapters per projection.
Both can be re-run layer by layer, so gradient checkpointing applies.  VLR_ILM_LORA_FUSED=0 replaces the second one by a layer composed
HERE from the library's bf16 primitives - the cross-check of the two-adapter calls: the projections run un-fused, the image rows are
gathered into a compact [R, in] matrix (vlr_gather_rows / vlr_rows_gather), run through two skinny GEMMs and added back (vlr_rows_add),
the peft adapters accumulate on all rows; bf16 residual stream, ~110 launches per layer and pass, activations kept (no checkpointing).
Dropout convention (the reference draws from torch's RNG): target t of layer l masks the compact [R, in] matrix with the counter-based
mask of vlr_dropout(seed + 8 l + t), t = 0 wqkv, 3 wo, 4 w1, 5 w3, 6 w2; PLoRA and LoRA use different seed bases."""
import math
import os

import torch

from . import _hip
from .engine import BF16, LlavaHipEngine

PLORA_T = dict(qkv=0, o=3, g=4, u=5, d=6)
PLORA_SEED_XOR = 0x2A5A5A5A5A


class InternLMHipEngine(LlavaHipEngine):
    # generate re-runs the forward per token unless the caller switches the cache on for THIS engine (InternLMXC2ForRL.enable_kv_cache
    # sets the instance attribute): then one prefill through _layer_fwd_call (PLoRA on the image rows) into a KVCache + decode_step.  A
    # new token is a text row - the PLoRA pairs add nothing to it (build_mlp.py:194-199; modeling_internlm2.py:787 builds a zero im_mask
    # when none is given) - so decode_step is the base engine's, on this family's weights.  The class default stays False.
    supports_kv_cache = False
    row_compact_layers = False     # the row-compact reference pass (forward_hidden(prefix_dedup_rows=True)) is not wired to this engine: dense passes only
    vision_prefix = "vit.vision_tower."

    @property
    def supports_ckpt(self):       # the C layer passes (full fine-tune / reference / LoRA over PLoRA) can be re-run; the Python-composed peft-LoRA layer keeps its activations
        return self.lora is None or self.lora_fused

    def __init__(self, cfg: dict, device="cuda", max_positions: int = 8192):
        c = dict(cfg, family="internlm_xc2")
        c.setdefault("vit_feature_layer", -1)
        c.setdefault("rope_theta", 1000000.0)
        super().__init__(c, device=device, max_positions=max_positions)
        self.plora_r = int(c.get("plora_r", 256))
        self.plora_scale = float(c.get("plora_alpha", 256)) / self.plora_r
        self.plora_p = float(c.get("plora_dropout", 0.05))
        self._plora_calls = 0
        self.plora_seed = int(c.get("seed", 0))
        self.lora_fused = False                  # set by enable_lora: peft LoRA over PLoRA on vlr_decoder_layer_*_lora2
        self.last_train_plora_seed = None        # PLoRA dropout seed of the last training-mode policy pass

    # ------------------------------------------------------------------------------------------------ decoding
    @staticmethod
    def kv_next_positions(key_mask, length=None):
        """the rotary position is the index in the merged sequence (_embed_inputs: pos = arange(S) in every row, padded or not): a row
        that was left-padded appends at position `length`, where the re-forward loop places it - not at its count of attended columns"""
        n = key_mask.shape[1] if length is None else int(length)
        return torch.full((key_mask.shape[0],), n, dtype=torch.int32, device=key_mask.device)

    @property
    def kv_cache_layers(self):
        """False while the decoder layers are the ones composed from bf16 primitives (peft LoRA under VLR_ILM_LORA_FUSED=0): they keep the
        re-forward loop.  Read when generate starts - enable_lora may run after the cache was switched on."""
        return self.lora is None or self.lora_fused

    def decode_step(self, ws, tokens, cache, lora=None):
        if not self.kv_cache_layers:
            raise ValueError("InternLMHipEngine: the composed bf16 layers (VLR_ILM_LORA_FUSED=0) have no KV-cache decoding")
        return super().decode_step(ws, tokens, cache, lora)

    # ------------------------------------------------------------------------------------------------ embed
    def _embed_inputs(self, ws, ids, am, lab, pixel_values, image_dup, tag, image_sizes, meta):
        e = super()._embed_inputs(ws, ids, am, lab, pixel_values, image_dup, tag, image_sizes, meta)
        Bn, S = ids.shape[0], e["S"]
        cached = meta.get("ilm") if meta is not None else None
        if cached is None:
            rows = e["img_map"].reshape(-1).nonzero().reshape(-1).to(torch.int32).contiguous()       # one D2H sync per batch (row count)
            cached = dict(rows=rows, R=int(rows.numel()),
                          pos=torch.arange(S, dtype=torch.int32, device=self.dev)[None].expand(Bn, S).contiguous())
            if meta is not None:
                meta["ilm"] = cached
        e["pos"] = cached["pos"]                       # rotary position = index in the merged sequence
        e["extra"] = cached
        self._plora_calls += 1                         # one PLoRA dropout stream per forward pass (a recompute re-uses the pass's seed)
        e["plora_seed"] = ((self.plora_seed << 40) + (self._plora_calls << 16)) ^ PLORA_SEED_XOR
        return e

    def enable_lora(self, r, alpha, dropout=0.0, seed=0):
        """peft LoRA stacked on the frozen PLoRA decoder (the configuration the reference ships for this family).  Default: the C layer
        passes with TWO adapters per projection (vlr_decoder_layer_fwd_lora2 / bwd_lora2, include/vlr.h) - fused qkv + RoPE / SwiGLU /
        residual projections, one adapter segment [B_lora | B_plora] in the K loop, fp32 residual stream.  VLR_ILM_LORA_FUSED=0 composes
        the layer from bf16 primitives instead (rows_add, accumulate GEMMs; bf16 residual stream) - the cross-check of the fused path."""
        super().enable_lora(r, alpha, dropout, seed)
        self.lora_fused = os.environ.get("VLR_ILM_LORA_FUSED", "1") != "0"
        if not self.lora_fused:
            self._to_bf16_stream()

    def _bcomb(self, ws, l):
        """[B_lora | B_plora] of layer l for the four fused projections (vlr_lora_bcomb): rebuilt from the live adapter weights in front
        of every layer pass (4 copies of 26 MB at the 7B shapes, ~10 us) so an optimizer step or a loaded adapter is never stale"""
        rl, rp = self.lora["r"], self.plora_r
        ptrs = []
        for grp, pk in (("qkv", "pb_qkv"), ("o", "pb_o"), ("gu", "pb_gu"), ("down", "pb_d")):
            Bl, Bp = self.lv[f"l{l}.b_{grp}"], ws.v[f"l{l}.{pk}"]
            rows = Bl.shape[0]
            out = self._buf(("bcomb", grp), (rows, rl + rp))
            _hip.call("vlr_lora_concat_b", Bl, rl, Bp, rp, out, rows)
            ptrs.append(out.data_ptr())
        return _hip.LoraBcomb(*ptrs)

    def _to_bf16_stream(self):
        if self.resid_f32:
            self.resid_f32, self.RDT = False, BF16
            self.llama_cfg = _hip.LlamaCfg(self.H, self.I, self.nh, self.hd, self.llama_cfg.rms_eps, self.max_pos, self.cos.data_ptr(),
                                           self.sin.data_ptr(), self.nkv, 0)
            self._ws = {}

    def _plora_structs(self, ws, l, p, M=None, acts=None):
        """the PLoRA pairs of layer l as the adapter structs of the C layer passes (include/vlr.h vlr_lora_weights): ONE adapter over the
        fused wqkv, wo, w1 | w3 stacked, w2; scale = alpha / r; gradients into the flat gradient buffer (full fine-tune) or nowhere"""
        v = ws.v
        names = ("pa_qkv", "pb_qkv", "pa_o", "pb_o", "pa_gu", "pb_gu", "pa_d", "pb_d")
        w = _hip.LoraWeights(self.plora_r, self.plora_scale, float(p), *(v[f"l{l}.{n}"].data_ptr() for n in names), 1,
                             self._mask_bits(l, M, float(p), acts, "plora_bits") if M else None)
        g = _hip.LoraGrads(*(self.gv[f"l{l}.{n}"].data_ptr() for n in names)) if self.gv is not None else None
        return w, g

    def _embed_backward(self, ctx, cur, acc):
        """the projector is frozen with the tower: only tok_embeddings receives a gradient in front of the decoder"""
        if not acc:
            self.gv["embed"].zero_()
        _hip.call("vlr_merge_bwd", cur, ctx["src"], ctx["inv"], ctx["ids"], None, self.gv["embed"], ctx["Bn"], ctx["T"], ctx["S"], self.H,
                  ctx["n_rows"], ctx["image_dup"])

    # ------------------------------------------------------------------------------------------------ adapters
    def _pab(self, views, l, key):
        """(Plora_A [r][in], Plora_B [out][r]) of target `key`; gate (w1) / up (w3) are the two halves of the stacked `gu` pair"""
        r, I = self.plora_r, self.I
        if key == "g":
            return views[f"l{l}.pa_gu"][:r], views[f"l{l}.pb_gu"][:I]
        if key == "u":
            return views[f"l{l}.pa_gu"][r:], views[f"l{l}.pb_gu"][I:]
        return views[f"l{l}.pa_{key}"], views[f"l{l}.pb_{key}"]

    def _gemm(self, layout, A, B, C, M, N, K, lda, ldb, ldc, residual=None, ldr=0, accumulate=0, alpha=1.0):
        _hip.call("vlr_gemm_bf16_scaled", layout, A, B, C, None, residual, M, N, K, lda, ldb, ldc, ldr, 0, accumulate, 0, float(alpha))

    def _plora_fwd(self, ws, l, key, x_in, n_in, y, ldy, n_out, ex, train, seed, tag):
        """y[img rows] += scale * (drop(x_in[img rows]) A^T) B^T;  y is a [M, n_out] column block with row stride ldy"""
        R, rows, r = ex["R"], ex["rows"], self.plora_r
        if R == 0:
            return
        A, B = self._pab(ws.v, l, key)
        xs = self._buf((tag, "pl_xs", R, n_in), (R, n_in))
        _hip.call("vlr_gather_rows", x_in, rows, xs, R, n_in)
        if train and self.plora_p > 0:
            _hip.call("vlr_dropout", xs, xs, R * n_in, self.plora_p, seed + PLORA_T[key], 1.0, 0)
        up = self._buf((tag, "pl_up", R), (R, r))
        self._gemm(0, xs, A, up, R, r, n_in, n_in, n_in, r, alpha=self.plora_scale)
        yp = self._buf((tag, "pl_y", R, n_out), (R, n_out))
        self._gemm(0, up, B, yp, R, n_out, r, r, r, n_out)
        _hip.call("vlr_rows_add", yp, rows, y, ldy, R, n_out)

    def _plora_bwd(self, ws, l, key, dy, lddy, n_out, dx, n_in, ex, train, seed):
        """dx[img rows] += the frozen PLoRA pair's input gradient"""
        R, rows, r = ex["R"], ex["rows"], self.plora_r
        if R == 0:
            return
        A, B = self._pab(ws.v, l, key)
        dyr = self._buf(("pl_dy", R, n_out), (R, n_out))
        _hip.call("vlr_rows_gather", dy, lddy, rows, dyr, R, n_out)
        v = self._buf(("pl_v", R), (R, r))
        self._gemm(1, dyr, B, v, R, r, n_out, n_out, r, r)                                   # v = dy B
        dxr = self._buf(("pl_dx", R, n_in), (R, n_in))
        self._gemm(1, v, A, dxr, R, n_in, r, r, n_in, n_in, alpha=self.plora_scale)
        if train and self.plora_p > 0:
            _hip.call("vlr_dropout", dxr, dxr, R * n_in, self.plora_p, seed + PLORA_T[key], 1.0, 0)
        _hip.call("vlr_rows_add", dxr, rows, dx, n_in, R, n_in)

    def _lora_fwd(self, l, grp, t, x_in, n_in, y, ldy, n_out, row0, seed, keep, M, tag):
        """peft adapter of sub-target t of group grp on ALL rows: y += (s drop(x) A_t^T) B_t^T"""
        lo = self.lora
        r = lo["r"]
        A = self.lv[f"l{l}.a_{grp}"][t * r:(t + 1) * r]
        B = self.lv[f"l{l}.b_{grp}"][row0:row0 + n_out]
        p = lo["dropout"] if self.training else 0.0
        xd = x_in
        if p > 0:
            xd = torch.empty(M, n_in, dtype=BF16, device=self.dev) if keep else self._buf((tag, "lo_xd", M, n_in), (M, n_in))
            _hip.call("vlr_dropout", x_in, xd, M * n_in, p, seed, 1.0, 0)
        u = torch.empty(M, r, dtype=BF16, device=self.dev) if keep else self._buf((tag, "lo_u", M), (M, r))
        self._gemm(0, xd, A, u, M, r, n_in, n_in, n_in, r, alpha=lo["scale"])
        self._gemm(0, u, B, y, M, n_out, r, r, r, ldy, accumulate=1)
        return (xd, u) if keep else None

    def _lora_bwd(self, l, grp, t, kept, dy, lddy, n_out, row0, dx, n_in, seed, acc, M):
        lo = self.lora
        r = lo["r"]
        A = self.lv[f"l{l}.a_{grp}"][t * r:(t + 1) * r]
        B = self.lv[f"l{l}.b_{grp}"][row0:row0 + n_out]
        xd, u = kept
        p = lo["dropout"] if self.training else 0.0
        self._gemm(2, dy, u, self.lgv[f"l{l}.b_{grp}"][row0:row0 + n_out], n_out, r, M, lddy, r, r, accumulate=acc)           # dB = dy^T (s u)
        v = self._buf(("lo_v", M), (M, r))
        self._gemm(1, dy, B, v, M, r, n_out, lddy, r, r)
        self._gemm(2, v, xd, self.lgv[f"l{l}.a_{grp}"][t * r:(t + 1) * r], r, n_in, M, r, n_in, n_in, accumulate=acc, alpha=lo["scale"])
        if p > 0:
            scratch = self._buf(("lo_dx", M, n_in), (M, n_in))
            _hip.call("vlr_gemm_dropout_acc", v, r, A, dx, scratch, M, n_in, r, p, seed, lo["scale"])
        else:
            self._gemm(1, v, A, dx, M, n_in, r, r, n_in, n_in, accumulate=1, alpha=lo["scale"])

    # ------------------------------------------------------------------------------------------------ layer forward
    def _targets(self):
        H, I, N = self.H, self.I, self.Nqkv
        #        key   lora group, sub-target, lora_B row0, in, out
        return dict(qkv=("qkv", 0, 0, H, N), o=("o", 0, 0, self.Nq, H), g=("gu", 0, 0, H, I), u=("gu", 1, I, H, I), d=("down", 0, 0, I, H))

    def _layer_fwd_call(self, ws, l, a, x, e, Bn, S, keep, use_lora, lora_seed):
        M = Bn * S
        train = self.training and ws is self.policy and bool(e.get("grad_pass", keep))     # (a checkpointed forward keeps nothing but is the same pass)
        pseed = e["plora_seed"]
        if train and l == 0:
            self.last_train_plora_seed = pseed       # (tests: the oracle regenerates the pass's masks from it)
        if keep:
            a["pseed"], a["train"] = pseed + 8 * l, train
        if use_lora and not self.lora_fused:
            return self._layer_fwd_composed(ws, l, a, x, e, Bn, S, keep, train, lora_seed)
        pw, _ = self._plora_structs(ws, l, self.plora_p if train else 0.0, M, a)
        if not use_lora:
            # only PLoRA sits on the linears (reference pass; policy pass of a full fine-tune): the C layer pass with the PLoRA pairs as
            # its adapters and the image rows as the row mask
            u = self._adapter_scratch(a, "u", M, 7 * self.plora_r)
            _hip.call("vlr_decoder_layer_fwd_lora_ex", self.llama_cfg, self.layer_weights(ws, l), pw, a["struct"], u, None,
                      pseed + 8 * l, e["img_map"], x, e["pos"], e["mask"], Bn, S)
        else:
            u2 = self._adapter_scratch(a, "u2", M, 7 * (self.lora["r"] + self.plora_r))
            lw, _ = self._lora_structs(l, train=True, M=M, acts=a)
            bc = self._bcomb(ws, l)
            _hip.call("vlr_decoder_layer_fwd_lora2", self.llama_cfg, self.layer_weights(ws, l), lw, pw, bc, a["struct"], u2,
                      lora_seed + 8 * l, pseed + 8 * l, e["img_map"], x, e["pos"], e["mask"], Bn, S)

    def _layer_fwd_composed(self, ws, l, a, x, e, Bn, S, save, train, lora_seed):
        """peft LoRA over the frozen PLoRA decoder from bf16 primitives (VLR_ILM_LORA_FUSED=0); save: keeps what _layer_bwd_composed reads"""
        c, H, I, N, M = self.llama_cfg, self.H, self.I, self.Nqkv, Bn * S
        ex, pos, mask, tag = e["extra"], e["pos"], e["mask"], e["tag"]
        pseed = e["plora_seed"] + 8 * l
        kept = {}
        tg = self._targets()

        def adapters(key, x_in, y, ldy):
            grp, t, row0, n_in, n_out = tg[key]
            self._plora_fwd(ws, l, key, x_in, n_in, y, ldy, n_out, ex, train, pseed, tag)
            kept[key] = self._lora_fwd(l, grp, t, x_in, n_in, y, ldy, n_out, row0, lora_seed + 8 * l + PLORA_T[key], save, M, tag)

        _hip.call("vlr_rmsnorm_fwd", x, ws.v[f"l{l}.ln1"], a["xn1"], a["rstd1"], M, H, c.rms_eps)
        self._gemm(0, a["xn1"], ws.v[f"l{l}.wqkv"], a["qkv"], M, N, H, H, H, N)
        adapters("qkv", a["xn1"], a["qkv"], N)
        _hip.call("vlr_rope_heads", a["qkv"], pos, self.cos, self.sin, M, self.nh + self.nkv, self.hd, N, self.max_pos, 0)
        _hip.call("vlr_attn_fwd_gqa", a["qkv"], a["qkv"][:, self.Nq:], a["qkv"][:, self.Nq + self.Nkv:], N, a["attn"], self.Nq, a["lse"], mask,
                  Bn, S, self.nh, self.nkv, self.hd, 1, 1.0 / math.sqrt(self.hd))
        self._gemm(0, a["attn"], ws.v[f"l{l}.wo"], a["x_mid"], M, H, self.Nq, self.Nq, self.Nq, H, residual=x, ldr=H)
        adapters("o", a["attn"], a["x_mid"], H)
        _hip.call("vlr_rmsnorm_fwd", a["x_mid"], ws.v[f"l{l}.ln2"], a["xn2"], a["rstd2"], M, H, c.rms_eps)
        self._gemm(0, a["xn2"], ws.v[f"l{l}.wgu"], a["gu"], M, 2 * I, H, H, H, 2 * I)
        adapters("g", a["xn2"], a["gu"], 2 * I)
        adapters("u", a["xn2"], a["gu"][:, I:], 2 * I)
        _hip.call("vlr_swiglu_fwd", a["gu"], a["act"], M, I)
        self._gemm(0, a["act"], ws.v[f"l{l}.wdown"], a["x_out"], M, H, I, I, I, H, residual=a["x_mid"], ldr=H)
        adapters("d", a["act"], a["x_out"], H)
        if save:
            a["kept"] = kept

    # ------------------------------------------------------------------------------------------------ backward
    def _layer_bwd(self, ctx, acc, wsb, lws):
        ws, Bn, S, M = ctx["ws"], ctx["Bn"], ctx["S"], ctx["M"]
        e = ctx["embed"]
        if self.lora is None:
            # full fine-tune: base AND PLoRA gradients, the adapters restricted to the image rows
            ws_v = self._buf(("plora_v", M), (M, 3 * self.plora_r))
            scratch = self._buf(("plora_scratch", M), (M, max(self.H, self.I)))

            def full(l, a, x_in, cur, nxt):
                pw, pg = self._plora_structs(ws, l, self.plora_p if a["train"] else 0.0, M, a)
                _hip.call("vlr_decoder_layer_bwd_lora_ex", self.llama_cfg, self.layer_weights(ws, l), self.layer_grads(l), pw, pg, acc,
                          a["struct"], a.get("shared", a)["u"], lws, ws_v, scratch, a["pseed"], e["img_map"], x_in, cur, nxt,
                          ctx["pos"], ctx["mask"], Bn, S)
            return full
        if not self.lora_fused:
            return self._layer_bwd_composed(ctx, acc, wsb)
        # peft LoRA over the frozen PLoRA decoder: gradients of the LoRA pairs only, dx through the base projections and BOTH adapters
        # (PLoRA on the image rows, its own dropout stream)
        ws_v = self._buf(("lora2_v", M), (M, 3 * (self.lora["r"] + self.plora_r)))

        def lora2(l, a, x_in, cur, nxt):
            lw, lg = self._lora_structs(l, train=True, M=M, acts=a)
            pw, _ = self._plora_structs(ws, l, self.plora_p if a["train"] else 0.0, M, a)
            bc = self._bcomb(ws, l)
            _hip.call("vlr_decoder_layer_bwd_lora2", self.llama_cfg, self.layer_weights(ws, l), lw, lg, pw, bc, acc, a["struct"],
                      a.get("shared", a)["u2"], lws, ws_v, ctx["lora_seed"] + 8 * l, a["pseed"], e["img_map"], x_in, cur, nxt,
                      ctx["pos"], ctx["mask"], Bn, S)
        return lora2

    def _layer_bwd_composed(self, ctx, acc, wsb):
        """backward of _layer_fwd_composed: gradients of the LoRA pairs, dx through the base projections and both adapters"""
        ws, Bn, S, M, H, I, N = ctx["ws"], ctx["Bn"], ctx["S"], ctx["M"], self.H, self.I, self.Nqkv
        ex = ctx["extra"]
        dact, dxn, dattn, dqkv, dx_mid, delta = (wsb[k] for k in ("dact", "dxn", "dattn", "dqkv", "dx_mid", "delta"))
        tg = self._targets()

        def composed(l, a, x_in, cur, nxt):
            kept, pseed, train = a["kept"], a["pseed"], a["train"]

            def adapters_bwd(key, dy, lddy, dx):
                grp, t, row0, n_in, n_out = tg[key]
                self._plora_bwd(ws, l, key, dy, lddy, n_out, dx, n_in, ex, train, pseed)
                self._lora_bwd(l, grp, t, kept[key], dy, lddy, n_out, row0, dx, n_in, ctx["lora_seed"] + 8 * l + PLORA_T[key], acc, M)

            # ---- MLP
            self._gemm(1, cur, ws.v[f"l{l}.wdown"], dact, M, I, H, H, I, I)
            adapters_bwd("d", cur, H, dact)
            _hip.call("vlr_swiglu_bwd", a["gu"], dact, M, I)                  # gu now holds [d gate | d up]
            self._gemm(1, a["gu"], ws.v[f"l{l}.wgu"], dxn, M, H, 2 * I, 2 * I, H, H)
            adapters_bwd("g", a["gu"], 2 * I, dxn)
            adapters_bwd("u", a["gu"][:, I:], 2 * I, dxn)
            _hip.call("vlr_rmsnorm_bwd", dxn, a["x_mid"], ws.v[f"l{l}.ln2"], a["rstd2"], cur, dx_mid, None, 0, self._norm_ws, M, H)
            # ---- attention
            self._gemm(1, dx_mid, ws.v[f"l{l}.wo"], dattn, M, self.Nq, H, H, self.Nq, self.Nq)
            adapters_bwd("o", dx_mid, H, dattn)
            _hip.call("vlr_attn_bwd_gqa", a["qkv"], a["qkv"][:, self.Nq:], a["qkv"][:, self.Nq + self.Nkv:], N, a["attn"], dattn, self.Nq, a["lse"],
                      delta, ctx["mask"], dqkv, dqkv[:, self.Nq:], dqkv[:, self.Nq + self.Nkv:], N, Bn, S, self.nh, self.nkv, self.hd, 1,
                      1.0 / math.sqrt(self.hd))
            _hip.call("vlr_rope_heads", dqkv, ctx["pos"], self.cos, self.sin, M, self.nh + self.nkv, self.hd, N, self.max_pos, 1)
            self._gemm(1, dqkv, ws.v[f"l{l}.wqkv"], dxn, M, H, N, N, H, H)
            adapters_bwd("qkv", dqkv, N, dxn)
            _hip.call("vlr_rmsnorm_bwd", dxn, x_in, ws.v[f"l{l}.ln1"], a["rstd1"], dx_mid, nxt, None, 0, self._norm_ws, M, H)
            a["kept"] = None
        return composed
