"""MI355X engine for the LLaVA-1.5 DPO step: owns the flat parameter / gradient / optimizer buffers and the
activation workspaces, and sequences libvlr_hip.so (include/vlr.h) for the forward, the backward and the optimizer.

PyTorch is used for device memory, streams and the autograd *boundary* only - every FLOP below goes through the C ABI.
There is no fallback path: without the HIP library (or a GPU) constructing the engine raises.

Replaces, for the DPO hot path, what the reference reaches through
  LlavaForRL.forward                    /root/reference/src/vlrlhf/models/Llava/__init__.py:111-271
  VLDPOTrainer.get_batch_logps          /root/reference/src/vlrlhf/base/trainer.py:148-188
  Trainer.training_step / optimizer     (transformers 4.41.0 + torch AdamW; flags scripts/dpo_llava.sh:35-41)
"""
import math
from typing import Dict, List, Optional

import torch

from . import _hip, gptq, prefix_dedup

BF16 = torch.bfloat16


def _align(n, a=8):
    return (n + a - 1) // a * a


def neftune_scale(alpha, T, H):
    """NEFTune magnitude m = alpha / sqrt(T * H) (transformers neftune_post_forward_hook: T = width of the input_ids the forward was
    handed) and the multiplier m * 2^-23 of include/vlr.h vlr_neftune_add, both rounded to fp32 once, as Python floats"""
    m = float(torch.tensor(float(alpha) / math.sqrt(float(T) * float(H)), dtype=torch.float32))
    return m, float(torch.tensor(m * 2.0 ** -23, dtype=torch.float32))


def qkv_row_perm(nh, nkv, hd):
    """InternLM2 stores the rows of its fused grouped-query wqkv per K/V head as [q_0..q_{g-1} | k | v]: the permutation that re-orders
    them to q | k | v blocks (engine row i = checkpoint row perm[i])"""
    g = nh // nkv
    idx = torch.arange((nh + 2 * nkv) * hd).view(nkv, g + 2, hd)
    return torch.cat([idx[:, :g].reshape(-1), idx[:, g].reshape(-1), idx[:, g + 1].reshape(-1)])


def invert_perm(perm):
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.numel())
    return inv


class ParamLayout:
    """Flat layout of the TRAINABLE parameters (LLM + projector; the vision tower is frozen, auto_load.py:554-555).

    Weight-decay region first, in the order the backward finishes them (lm_head, layer L-1 .. 0, projector,
    embed_tokens) so contiguous slices are the DDP buckets; then the no-decay region (norm weights, biases).

    cfg["train_vision_tower"] (--freeze_vision_tower False, LLaVA-1.5 / LLaVA-Next): the CLIP tower's EVALUATED tensors join - the
    embeddings, pre_layrnorm and encoder layers 0 .. vit_layers + vit_feature_layer (q|k|v fused as VisionWeights fuses them).  The
    weight matrices, class_embedding and position_embedding.weight close the decay region (the backward finishes them last: they
    ride the last DDP bucket), the LayerNorm weights and the biases the no-decay region - the split of HF's decay grouping.  The
    never-evaluated last layer and post_layernorm get no gradient in the reference either: they stay in the frozen copy."""

    def __init__(self, cfg):
        H, I, V, D, L = cfg["hidden"], cfg["inter"], cfg["vocab"], cfg.get("vit_hidden", 8), cfg["layers"]
        assert H % 8 == 0 and I % 8 == 0 and V % 8 == 0 and D % 8 == 0
        nh = cfg.get("heads") or 1
        nkv = cfg.get("kv_heads") or nh                       # grouped-query attention (Mistral, InternLM2)
        hd = cfg.get("head_dim") or H // nh
        Nq, Nkv = nh * hd, nkv * hd
        self.entries = []   # (name, shape, [(hf_name, row0, rows)])
        e = self.entries
        qwen = cfg.get("family") == "qwen_vl"
        ilm = cfg.get("family") == "internlm_xc2"
        tower = bool(cfg.get("train_vision_tower"))
        if tower and (qwen or ilm):
            raise NotImplementedError(f"train_vision_tower: {'Qwen-VL' if qwen else 'InternLM-XComposer2'} has no vision-tower backward "
                                      "(LLaVA-1.5 and LLaVA-Next only)")
        self.col_pad = {}           # entry name -> checkpoint shape behind the rows: loaded flattened into the first prod(shape) columns
        self.row_perm = {}          # entry name -> row permutation applied when loading (engine row i = checkpoint row perm[i])
        if ilm:
            # InternLM-XComposer2 (reference models/InternLMXC2/modeling_internlm2.py): fused grouped-query wqkv with rows laid out per
            # K/V head as [q_0..q_{g-1} | k | v] (re-ordered to q | k | v blocks at load time), w2(silu(w1(x)) * w3(x)), and a PLoRA pair
            # (build_mlp.py:158-203) on every linear - base-model weights, trained by a full fine-tune
            lm, layer = "", "model.layers.{}."
            nm = dict(lm_head="output.weight", embed="model.tok_embeddings.weight", norm="model.norm.weight", down="feed_forward.w2.weight",
                      gate="feed_forward.w1.weight", up="feed_forward.w3.weight", o="attention.wo.weight", ln1="attention_norm.weight",
                      ln2="ffn_norm.weight")
            qkv_perm = qkv_row_perm(nh, nkv, hd)
        elif qwen:
            # Qwen-VL (reference models/QwenVL/modeling_qwen.py): fused biased c_attn, MLP c_proj(w1(x) * silu(w2(x))) -> gate = w2,
            # up = w1; no projector (the resampler is part of the frozen vision tower)
            lm, layer = "", "transformer.h.{}."
            nm = dict(lm_head="lm_head.weight", embed="transformer.wte.weight", norm="transformer.ln_f.weight", down="mlp.c_proj.weight",
                      gate="mlp.w2.weight", up="mlp.w1.weight", o="attn.c_proj.weight", ln1="ln_1.weight", ln2="ln_2.weight")
        else:
            lm, layer = "language_model.", "language_model.model.layers.{}."
            nm = dict(lm_head=lm + "lm_head.weight", embed=lm + "model.embed_tokens.weight", norm=lm + "model.norm.weight",
                      down="mlp.down_proj.weight", gate="mlp.gate_proj.weight", up="mlp.up_proj.weight", o="self_attn.o_proj.weight",
                      ln1="input_layernorm.weight", ln2="post_attention_layernorm.weight")
        e.append(("lm_head", (V, H), [(nm["lm_head"], 0, V)]))
        for l in range(L - 1, -1, -1):
            p = layer.format(l)
            e.append((f"l{l}.wdown", (H, I), [(p + nm["down"], 0, H)]))
            e.append((f"l{l}.wgu", (2 * I, H), [(p + nm["gate"], 0, I), (p + nm["up"], I, I)]))
            e.append((f"l{l}.wo", (H, Nq), [(p + nm["o"], 0, H)]))
            if qwen:
                e.append((f"l{l}.wqkv", (Nq + 2 * Nkv, H), [(p + "attn.c_attn.weight", 0, Nq + 2 * Nkv)]))
            elif ilm:
                pr = int(cfg.get("plora_r", 256))
                e.append((f"l{l}.wqkv", (Nq + 2 * Nkv, H), [(p + "attention.wqkv.weight", 0, Nq + 2 * Nkv)]))
                self.row_perm[f"l{l}.wqkv"] = qkv_perm
                for key, mod, din, dout in (("qkv", "attention.wqkv", H, Nq + 2 * Nkv), ("o", "attention.wo", Nq, H), ("d", "feed_forward.w2", I, H)):
                    e.append((f"l{l}.pa_{key}", (pr, din), [(p + mod + ".Plora_A.weight", 0, pr)]))
                    e.append((f"l{l}.pb_{key}", (dout, pr), [(p + mod + ".Plora_B.weight", 0, dout)]))
                # gate (w1) and up (w3): Plora_A stacked [2r][H], Plora_B stacked [2I][r] like the fused gate|up weight, so that the pair
                # can ride the K loop of the fused SwiGLU GEMM as its adapter segment
                e.append((f"l{l}.pa_gu", (2 * pr, H), [(p + "feed_forward.w1.Plora_A.weight", 0, pr), (p + "feed_forward.w3.Plora_A.weight", pr, pr)]))
                e.append((f"l{l}.pb_gu", (2 * I, pr), [(p + "feed_forward.w1.Plora_B.weight", 0, I), (p + "feed_forward.w3.Plora_B.weight", I, I)]))
                self.row_perm[f"l{l}.pb_qkv"] = qkv_perm
            else:
                e.append((f"l{l}.wqkv", (Nq + 2 * Nkv, H), [(p + "self_attn.q_proj.weight", 0, Nq), (p + "self_attn.k_proj.weight", Nq, Nkv),
                                                            (p + "self_attn.v_proj.weight", Nq + Nkv, Nkv)]))
        self.tail_start = "embed" if (qwen or ilm) else "proj.w2"
        if not (qwen or ilm):
            e.append(("proj.w2", (H, H), [("multi_modal_projector.linear_2.weight", 0, H)]))
            e.append(("proj.w1", (H, D), [("multi_modal_projector.linear_1.weight", 0, H)]))
        if cfg.get("image_grid_pinpoints"):                   # LLaVA-Next: the row appended to every line of the un-padded tile grid
            e.append(("image_newline", (H,), [("image_newline", 0, H)]))
        e.append(("embed", (V, H), [(nm["embed"], 0, V)]))
        if tower:
            vp = "vision_tower.vision_model."
            Fv, Pz = cfg["vit_mlp"], cfg["patch_size"]
            self.vit_layers = cfg["vit_layers"] + 1 + int(cfg.get("vit_feature_layer", -2))      # the layers the forward evaluates
            Tv = (cfg["image_size"] // Pz) ** 2 + 1
            for i in range(self.vit_layers - 1, -1, -1):
                p = f"{vp}encoder.layers.{i}."
                e.append((f"vit.l{i}.w2", (D, Fv), [(p + "mlp.fc2.weight", 0, D)]))
                e.append((f"vit.l{i}.w1", (Fv, D), [(p + "mlp.fc1.weight", 0, Fv)]))
                e.append((f"vit.l{i}.wo", (D, D), [(p + "self_attn.out_proj.weight", 0, D)]))
                e.append((f"vit.l{i}.wqkv", (3 * D, D), [(p + f"self_attn.{n_}_proj.weight", j * D, D) for j, n_ in enumerate("qkv")]))
            e.append(("vit.pos", (Tv, D), [(vp + "embeddings.position_embedding.weight", 0, Tv)]))
            e.append(("vit.cls", (D,), [(vp + "embeddings.class_embedding", 0, D)]))
            e.append(("vit.patch_w", (D, _align(3 * Pz * Pz, 8)), [(vp + "embeddings.patch_embedding.weight", 0, D)]))      # K-padded like VisionWeights.patch_w
            self.col_pad["vit.patch_w"] = (3, Pz, Pz)
        ap = "transformer.visual.attn_pool."
        if qwen and cfg.get("visual"):
            # the resampler of the Qwen-VL vision tower stays trainable in a full fine-tune (QwenVLForRL.freeze_vision_tower,
            # reference models/QwenVL/__init__.py:33-37): its weights live in the trainable buffer; the ViT trunk, ln_post and proj do not
            vq = cfg["visual"]
            E_, W_, nq_ = vq["output_dim"], vq["width"], int(vq.get("n_queries", 256))
            e.append(("ap.win", (3 * E_, E_), [(ap + "attn.in_proj_weight", 0, 3 * E_)]))
            e.append(("ap.wo", (E_, E_), [(ap + "attn.out_proj.weight", 0, E_)]))
            e.append(("ap.kv", (E_, W_), [(ap + "kv_proj.weight", 0, E_)]))
            e.append(("ap.query", (nq_, E_), [(ap + "query", 0, nq_)]))
        # HF Trainer.get_decay_parameter_names excludes nn.LayerNorm / LlamaRMSNorm (ALL_LAYERNORM_LAYERS) and `bias` parameters from weight
        # decay.  The RMSNorm classes VENDORED with Qwen-VL (modeling_qwen.py) and InternLM2 (modeling_internlm2.py) are not in that list:
        # the reference decays their weights (weight_decay 0.05 / 0.1 in the shipped scripts), so for these families the norm weights
        # sit in the decay region and only biases (and the resampler's nn.LayerNorm weights) stay outside it.
        norms_decay = qwen or ilm
        def _norms():
            e.append(("norm", (H,), [(nm["norm"], 0, H)]))
            for l in range(L - 1, -1, -1):
                p = layer.format(l)
                e.append((f"l{l}.ln2", (H,), [(p + nm["ln2"], 0, H)]))
                e.append((f"l{l}.ln1", (H,), [(p + nm["ln1"], 0, H)]))
        if norms_decay:
            _norms()
        # reward model (cfg["rm_head"]; reference base/model.py VLRewardModel: rm_head = nn.Linear(hidden, 1)): the weight closes the
        # decay region, the bias the no-decay region - the clip, AdamW, the DDP tail bucket and the optimizer checkpoint cover both.
        # Neither is part of the base model's checkpoint (no hf name): they travel in rm_head.bin
        rm_head = bool(cfg.get("rm_head"))
        if rm_head:
            e.append(("rm_head.w", (H,), []))
        # PPO value head (cfg["v_head"]; trl AutoModelForCausalLMWithValueHead: v_head.summary = nn.Linear(hidden, 1) on every position): placed
        # exactly as the reward head is, weight in the decay region and bias outside it (PPO steps with weight decay 0 either way)
        v_head = bool(cfg.get("v_head"))
        if v_head and rm_head:
            raise ValueError("cfg['rm_head'] and cfg['v_head'] on one engine: the reward model and the PPO policy are separate models")
        if v_head:
            e.append(("v_head.w", (H,), []))
        self.n_decay_entries = len(e)
        if not norms_decay:
            _norms()
        for l in range(L - 1, -1, -1):
            p = layer.format(l)
            if qwen:
                e.append((f"l{l}.bqkv", (Nq + 2 * Nkv,), [(p + "attn.c_attn.bias", 0, Nq + 2 * Nkv)]))
        if qwen and cfg.get("visual"):
            E_ = cfg["visual"]["output_dim"]
            e.append(("ap.bin", (3 * E_,), [(ap + "attn.in_proj_bias", 0, 3 * E_)]))
            e.append(("ap.bo", (E_,), [(ap + "attn.out_proj.bias", 0, E_)]))
            for k_, n_ in (("lnq_w", "ln_q.weight"), ("lnq_b", "ln_q.bias"), ("lnkv_w", "ln_kv.weight"), ("lnkv_b", "ln_kv.bias")):
                e.append((f"ap.{k_}", (E_,), [(ap + n_, 0, E_)]))
        if not (qwen or ilm):
            e.append(("proj.b2", (H,), [("multi_modal_projector.linear_2.bias", 0, H)]))
            e.append(("proj.b1", (H,), [("multi_modal_projector.linear_1.bias", 0, H)]))
        if tower:
            for i in range(self.vit_layers - 1, -1, -1):
                p = f"{vp}encoder.layers.{i}."
                for k_, n_, w_ in (("b2", "mlp.fc2.bias", D), ("b1", "mlp.fc1.bias", Fv), ("ln2_w", "layer_norm2.weight", D), ("ln2_b", "layer_norm2.bias", D),
                                   ("bo", "self_attn.out_proj.bias", D), ("ln1_w", "layer_norm1.weight", D), ("ln1_b", "layer_norm1.bias", D)):
                    e.append((f"vit.l{i}.{k_}", (w_,), [(p + n_, 0, w_)]))
                e.append((f"vit.l{i}.bqkv", (3 * D,), [(p + f"self_attn.{n_}_proj.bias", j * D, D) for j, n_ in enumerate("qkv")]))
            e.append(("vit.pre_w", (D,), [(vp + "pre_layrnorm.weight", 0, D)]))
            e.append(("vit.pre_b", (D,), [(vp + "pre_layrnorm.bias", 0, D)]))
        if rm_head:
            e.append(("rm_head.b", (1,), []))
        if v_head:
            e.append(("v_head.b", (1,), []))
        self.n_trainable_entries = len(e)
        if ilm:      # --freeze_vision_tower freezes the projector too (InternLMXC2/__init__.py:252-255): kept OUTSIDE the optimizer's range
            e.append(("proj.w2", (H, H), [("vision_proj.2.weight", 0, H)]))
            e.append(("proj.w1", (H, D), [("vision_proj.0.weight", 0, H)]))
            e.append(("proj.b2", (H,), [("vision_proj.2.bias", 0, H)]))
            e.append(("proj.b1", (H,), [("vision_proj.0.bias", 0, H)]))
        # GPTQ base (cfg["gptq"], q_lora): the decoder projections live packed outside the flat buffer (engine.packed) and take no room
        # in it - they keep their entry (names, shapes, fused row order) so that the packed loader stacks the parts the same way
        self.packed = {name for name, _, _ in e if gptq.is_packed_entry(name)} if cfg.get("gptq") else set()
        self.offset = {}
        off = 0
        self.n_opt = None
        for i, (name, shape, _) in enumerate(e):
            if i == self.n_decay_entries:
                self.n_decay = off
            if i == self.n_trainable_entries:
                self.n_opt = off
            self.offset[name] = off
            if name not in self.packed:
                off += _align(int(math.prod(shape)))
        self.numel = off
        if self.n_opt is None:
            self.n_opt = off           # elements [0, n_opt) are trainable (optimizer, gradient norm, DDP buckets); the rest is frozen
        self.shape = {name: shape for name, shape, _ in e}
        # DDP buckets = contiguous slices of the flat gradient in backward-completion order
        self.bucket_after = {}   # event name -> (start, end)
        ts = self.offset[self.tail_start]
        self.bucket_after["lm_head"] = (0, self.offset[f"l{L - 1}.wdown"] if L else ts)
        for l in range(L - 1, -1, -1):
            end = self.offset[f"l{l - 1}.wdown"] if l > 0 else ts
            self.bucket_after[f"layer{l}"] = (self.offset[f"l{l}.wdown"], end)
        self.bucket_after["tail"] = (ts, self.n_opt)

    def hf_names(self):
        for name, shape, parts in self.entries:
            if name in self.packed:
                continue
            for hf, r0, rows in parts:
                yield hf, name, r0, rows

    def views(self, flat):
        """named views of a flat buffer with this layout (packed entries have none)"""
        return {n: flat[self.offset[n]: self.offset[n] + int(math.prod(s))].view(*s) for n, s in self.shape.items() if n not in self.packed}


LORA_KEYS = ("a_qkv", "b_qkv", "a_o", "b_o", "a_gu", "b_gu", "a_down", "b_down")
# (group, peft module path, sub-target names in stacking order)
LORA_GROUPS = (("qkv", "self_attn", ("q_proj", "k_proj", "v_proj")), ("o", "self_attn", ("o_proj",)),
               ("gu", "mlp", ("gate_proj", "up_proj")), ("down", "mlp", ("down_proj",)))
LORA_TARGETS = tuple(t for _, _, ts in LORA_GROUPS for t in ts)
# Qwen-VL (QwenVLForRL.default_lora_target, reference models/QwenVL/__init__.py:26-28): ONE adapter over the fused c_attn, attn.c_proj,
# w2 (= gate) and w1 (= up); mlp.c_proj has none
QWEN_LORA_GROUPS = (("qkv", "attn", ("c_attn",)), ("o", "attn", ("c_proj",)), ("gu", "mlp", ("w2", "w1")))
# InternLM-XComposer2 (InternLMXC2ForRL.default_lora_target, reference models/InternLMXC2/__init__.py:244-245): peft adapters on the five
# PLoRA linears - one over the fused grouped-query wqkv (lora_B rows in the checkpoint's per-K/V-head order)
ILM_LORA_GROUPS = (("qkv", "attention", ("wqkv",)), ("o", "attention", ("wo",)), ("gu", "feed_forward", ("w1", "w3")), ("down", "feed_forward", ("w2",)))


class LoraLayout:
    """Flat bf16 layout of the peft adapters on the decoder linears.  LLaVA / LLaVA-Next (LlavaForRL.default_lora_target,
    /root/reference src/vlrlhf/models/Llava/__init__.py:273-286), per layer: a_qkv [3r,H] | b_qkv [3H,r] | a_o [r,H] | b_o [H,r] |
    a_gu [2r,H] | b_gu [2I,r] | a_down [r,I] | b_down [H,r]; Qwen-VL: a_qkv [r,H] | b_qkv [3H,r] | a_o | b_o | a_gu | b_gu.
    Sub-targets of a fused group are stacked rows, matching vlr_lora_weights (include/vlr.h)."""

    def __init__(self, cfg, r):
        H, I, L = cfg["hidden"], cfg["inter"], cfg["layers"]
        nh = cfg.get("heads") or 1
        nkv = cfg.get("kv_heads") or nh
        hd = cfg.get("head_dim") or H // nh
        Nq, Nkv = nh * hd, nkv * hd
        self.r, self.L = r, L
        self.qwen = cfg.get("family") == "qwen_vl"
        self.row_perm = {}
        if cfg.get("family") == "internlm_xc2":
            self.groups, self.prefix = ILM_LORA_GROUPS, "base_model.model.model.layers."
            per = dict(a_qkv=(r, H), b_qkv=(Nq + 2 * Nkv, r), a_o=(r, Nq), b_o=(H, r), a_gu=(2 * r, H), b_gu=(2 * I, r), a_down=(r, I), b_down=(H, r))
            self.out_dim = dict(wqkv=Nq + 2 * Nkv, wo=H, w1=I, w3=I, w2=H)
            self.row_perm["b_qkv"] = qkv_row_perm(nh, nkv, hd)
        elif self.qwen:
            self.groups, self.prefix = QWEN_LORA_GROUPS, "base_model.model.transformer.h."
            per = dict(a_qkv=(r, H), b_qkv=(Nq + 2 * Nkv, r), a_o=(r, Nq), b_o=(H, r), a_gu=(2 * r, H), b_gu=(2 * I, r))
            self.out_dim = dict(c_attn=Nq + 2 * Nkv, c_proj=H, w2=I, w1=I)
        else:
            self.groups, self.prefix = LORA_GROUPS, "base_model.model.language_model.model.layers."
            per = dict(a_qkv=(3 * r, H), b_qkv=(Nq + 2 * Nkv, r), a_o=(r, Nq), b_o=(H, r), a_gu=(2 * r, H), b_gu=(2 * I, r),
                       a_down=(r, I), b_down=(H, r))
            self.out_dim = dict(q_proj=Nq, k_proj=Nkv, v_proj=Nkv, o_proj=H, gate_proj=I, up_proj=I, down_proj=H)
        self.keys = tuple(k for k in LORA_KEYS if k in per)
        self.qkv_targets = 1 if (self.qwen or cfg.get("family") == "internlm_xc2") else 3
        self.offset, self.shape = {}, {}
        o = 0
        for l in range(L):
            for k in self.keys:
                self.offset[f"l{l}.{k}"] = o
                self.shape[f"l{l}.{k}"] = per[k]
                o += _align(per[k][0] * per[k][1])
        self.n_decay = o          # [n_decay, numel): stepped with weight decay 0 (the reward head's bias; empty without cfg["rm_head"])
        if cfg.get("rm_head"):    # the reward head trains beside the adapters (peft modules_to_save=["rm_head"]): weight, then bias
            self.offset["rm_head.w"], self.shape["rm_head.w"] = o, (H,)
            o += _align(H)
            self.n_decay = o
            self.offset["rm_head.b"], self.shape["rm_head.b"] = o, (1,)
            o += _align(1)
        if cfg.get("v_head"):     # the PPO value head trains beside the adapters the same way (ParamLayout refuses both heads at once)
            self.offset["v_head.w"], self.shape["v_head.w"] = o, (H,)
            o += _align(H)
            self.n_decay = o
            self.offset["v_head.b"], self.shape["v_head.b"] = o, (1,)
            o += _align(1)
        self.numel = o

    def hf_names(self, prefix=None):
        """peft adapter-file name -> (flat key, row_lo, row_hi)"""
        prefix = self.prefix if prefix is None else prefix
        out = {}
        r = self.r
        for l in range(self.L):
            for g, mod, ts in self.groups:
                row = 0
                for i, t in enumerate(ts):
                    od = self.out_dim[t]
                    out[f"{prefix}{l}.{mod}.{t}.lora_A.weight"] = (f"l{l}.a_{g}", i * r, (i + 1) * r)
                    out[f"{prefix}{l}.{mod}.{t}.lora_B.weight"] = (f"l{l}.b_{g}", row, row + od)
                    row += od
        return out


class WeightSet:
    """One set of LLM + projector weights in a flat bf16 buffer, with named 2-D views."""

    def __init__(self, layout: ParamLayout, device, flat: Optional[torch.Tensor] = None):
        self.layout = layout
        self.flat = flat if flat is not None else torch.zeros(layout.numel, dtype=BF16, device=device)
        self.version = 0          # bumped by load_state_dict (caches derived from the weights key on it)
        self.v = layout.views(self.flat)

    def clone(self):
        return WeightSet(self.layout, self.flat.device, self.flat.clone())

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict=True):
        self.version += 1
        seen = set()
        for hf, name, r0, rows in self.layout.hf_names():
            if hf not in sd:
                if strict:
                    raise KeyError(f"missing weight {hf}")
                continue
            t = sd[hf]
            dst = self.v[name]
            perm = self.layout.row_perm.get(name)
            if perm is not None:
                t = t[perm.to(t.device)]
            if name in self.layout.col_pad:      # [rows, *shape] in the checkpoint, flattened into the leading columns (the rest stay zero)
                dst[r0:r0 + rows, :int(math.prod(self.layout.col_pad[name]))].copy_(t.to(BF16).reshape(rows, -1))
            elif dst.dim() == 1 and rows == dst.shape[0]:
                dst.copy_(t.to(BF16))
            else:
                dst[r0:r0 + rows].copy_(t.to(BF16))
            seen.add(hf)
        return seen

    def state_dict(self):
        out = {}
        for hf, name, r0, rows in self.layout.hf_names():
            v = self.v[name]
            perm = self.layout.row_perm.get(name)
            if perm is not None:                  # back to the checkpoint's row order (a copy, not a view)
                out[hf] = v[invert_perm(perm).to(v.device)]
                continue
            if name in self.layout.col_pad:      # back to the checkpoint's shape (splitting the column dimension: still a view)
                shp = self.layout.col_pad[name]
                out[hf] = v[r0:r0 + rows, :int(math.prod(shp))].reshape(rows, *shp)
                continue
            out[hf] = v if (v.dim() == 1 and rows == v.shape[0]) else v[r0:r0 + rows]
        return out


class VisionWeights:
    """Frozen CLIP ViT weights, bf16, q|k|v fused, patch-embedding kernel flattened and K-padded to a multiple of 8."""

    def __init__(self, cfg, sd, device, prefix="vision_tower.vision_model."):
        D, P = cfg["vit_hidden"], cfg["patch_size"]
        self.Kp = _align(3 * P * P, 8)
        dv = lambda t: t.to(BF16).to(device).contiguous()  # noqa: E731
        w = torch.zeros(D, self.Kp)
        w[:, : 3 * P * P] = sd[prefix + "embeddings.patch_embedding.weight"].float().reshape(D, -1)
        self.patch_w = dv(w)
        self.cls = dv(sd[prefix + "embeddings.class_embedding"].reshape(D))
        self.pos = dv(sd[prefix + "embeddings.position_embedding.weight"])
        self.pre_w, self.pre_b = dv(sd[prefix + "pre_layrnorm.weight"]), dv(sd[prefix + "pre_layrnorm.bias"])
        self.layers = []
        self._keep = []
        for i in range(cfg["vit_layers"] + 1 + int(cfg.get("vit_feature_layer", -2))):   # vision_feature_layer -2 (LLaVA): the last layer is never evaluated; -1: all
            p = f"{prefix}encoder.layers.{i}."
            t = dict(
                ln1_w=dv(sd[p + "layer_norm1.weight"]), ln1_b=dv(sd[p + "layer_norm1.bias"]),
                wqkv=dv(torch.cat([sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], 0)),
                bqkv=dv(torch.cat([sd[p + f"self_attn.{n}_proj.bias"] for n in "qkv"], 0)),
                wo=dv(sd[p + "self_attn.out_proj.weight"]), bo=dv(sd[p + "self_attn.out_proj.bias"]),
                ln2_w=dv(sd[p + "layer_norm2.weight"]), ln2_b=dv(sd[p + "layer_norm2.bias"]),
                w1=dv(sd[p + "mlp.fc1.weight"]), b1=dv(sd[p + "mlp.fc1.bias"]),
                w2=dv(sd[p + "mlp.fc2.weight"]), b2=dv(sd[p + "mlp.fc2.bias"]))
            self._keep.append(t)
            self.layers.append(_hip.VitLayerWeights(*(t[k].data_ptr() for k in (
                "ln1_w", "ln1_b", "wqkv", "bqkv", "wo", "bo", "ln2_w", "ln2_b", "w1", "b1", "w2", "b2"))))


VIT_KEYS = ("ln1_w", "ln1_b", "wqkv", "bqkv", "wo", "bo", "ln2_w", "ln2_b", "w1", "b1", "w2", "b2")


class TowerViews:
    """A CLIP tower whose tensors are the "vit.*" views of a flat buffer laid out by ParamLayout(train_vision_tower): the trainable
    tower over the policy weights (struct = vlr_vit_layer_weights) or its gradients (vlr_vit_layer_grads).  Same attributes as
    VisionWeights; the views alias the flat buffer, so an optimizer step or a reload moves the tower with it."""

    def __init__(self, views, n_layers, struct):
        self.patch_w, self.cls, self.pos = views["vit.patch_w"], views["vit.cls"], views["vit.pos"]
        self.pre_w, self.pre_b = views["vit.pre_w"], views["vit.pre_b"]
        self.Kp = self.patch_w.shape[1]
        self.layers = [struct(*(views[f"vit.l{i}.{k}"].data_ptr() for k in VIT_KEYS)) for i in range(n_layers)]


class KVCache:
    """Per-layer K / V cache of `generate` with use_cache (transformers DynamicCache): k, v [L][B][kv_heads][cap][head_dim] bf16 (post-RoPE,
    written by the prefill - LlavaHipEngine.forward_hidden(kv_cache=...) - and one column per decode step), key_mask [B][cap] int32
    (0 = padded key, the merge's convention), `len` = filled columns (the same for every row), `pos` [B] int32 = each row's NEXT position.

    Positions follow the merge (cumsum(mask) - 1 on the attended rows), so a new token's position is the number of attended columns of
    its row - unless the engine that made the cache says otherwise: `position_rule` (engine.kv_next_positions, set by
    engine.new_kv_cache / new_shared_kv_cache; None = the rule above) gives the first new token's position from the mask.
    The buffers are allocated by `reserve(S)` once the prompt's merged length S is known: capacity = S + `new_tokens`."""

    def __init__(self, layers, batch, kv_heads, head_dim, new_tokens, device="cuda"):
        self.L, self.B, self.kv_heads, self.head_dim = int(layers), int(batch), int(kv_heads), int(head_dim)
        self.new_tokens = int(new_tokens)
        self.device = torch.device(device)
        self.cap = 0
        self.len = 0
        self.k = self.v = self.key_mask = self.pos = None
        self.position_rule = None

    @staticmethod
    def capacity(prompt_len, new_tokens):
        """columns the cache needs: the merged prompt plus one per new token"""
        return int(prompt_len) + int(new_tokens)

    @staticmethod
    def next_positions(key_mask, length=None):
        """[B] int32: position of the token each row appends next = attended columns among the first `length`"""
        m = key_mask if length is None else key_mask[:, :length]
        return (m != 0).sum(1).to(torch.int32)

    def reserve(self, prompt_len, alloc=True):
        self.cap = self.capacity(prompt_len, self.new_tokens)
        self.len = 0
        self.key_mask = torch.zeros(self.B, self.cap, dtype=torch.int32, device=self.device)
        self.pos = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        if alloc:
            shape = (self.L, self.B, self.kv_heads, self.cap, self.head_dim)
            self.k = torch.empty(shape, dtype=BF16, device=self.device)
            self.v = torch.empty(shape, dtype=BF16, device=self.device)
        return self.cap

    def start(self, mask):
        """the prefill filled columns [0, S) with the merged rows of attention mask `mask` [B][S]"""
        S = mask.shape[1]
        if S > self.cap:
            raise ValueError(f"KV cache: prompt of {S} merged rows exceeds the capacity {self.cap}")
        self.key_mask[:, :S] = mask.to(device=self.key_mask.device, dtype=torch.int32)
        self.len = S
        self.pos = (self.position_rule or self.next_positions)(self.key_mask, S).to(torch.int32).contiguous()

    def open_column(self):
        """marks column `len` (the token of the coming decode step) as attended in every row; -> that column"""
        if self.len >= self.cap:
            raise ValueError(f"KV cache full: {self.len} of {self.cap} columns filled")
        self.key_mask[:, self.len] = 1
        return self.len

    def advance(self):
        self.len += 1
        self.pos += 1


class SharedPromptKVCache:
    """K / V cache of `generate(num_return_sequences=n)`: the `fanout` = n samples of a prompt share ONE copy of the prompt's K / V.

    prompt   a KVCache(new_tokens=0) of the P prompts, filled by the unchanged prefill (forward_hidden(kv_cache=cache.prompt)); never
             written again.
    tail     k_tail, v_tail [L][P*n][kv_heads][new_tokens][head_dim] bf16: the samples' own new tokens, one column per decode step.  Row
             p*n + j is sample j of prompt p (the order of repeat_interleave).  Every tail column below `tail_len` is attended - finished
             rows keep receiving pad tokens, as in KVCache - so the tail has no mask.
    pos      [P*n] int32: each sample's NEXT position = the prompt's next position repeated n times, then + 1 per step.
    `begin()` is called once after the prefill; open_column() / advance() bracket a decode step as KVCache's do."""

    def __init__(self, layers, prompts, fanout, kv_heads, head_dim, new_tokens, device="cuda"):
        if int(fanout) < 1:
            raise ValueError(f"SharedPromptKVCache: fanout {fanout} must be at least 1")
        self.prompt = KVCache(layers, prompts, kv_heads, head_dim, 0, device)
        self.L, self.P, self.fanout, self.B = int(layers), int(prompts), int(fanout), int(prompts) * int(fanout)
        self.kv_heads, self.head_dim, self.new_tokens = int(kv_heads), int(head_dim), int(new_tokens)
        self.device = torch.device(device)
        self.tail_cap = self.new_tokens
        self.tail_len = 0
        self.k_tail = self.v_tail = self.pos = None

    @property
    def cap(self):
        """columns a sample can attend: the prompt's capacity plus its own tail's"""
        return self.prompt.cap + self.tail_cap

    @property
    def len(self):
        return self.prompt.len + self.tail_len

    def nbytes(self):
        """bytes of K / V held (prompt once, tails per sample)"""
        return 2 * 2 * self.L * self.kv_heads * self.head_dim * (self.P * self.prompt.cap + self.B * self.tail_cap)

    def begin(self, alloc=True):
        """after the prefill: empty tails, and every sample starts at its prompt's next position (the prompt cache's position_rule)"""
        if self.prompt.len < 1:
            raise ValueError("SharedPromptKVCache.begin: the prompt segment is empty (run the prefill first)")
        self.tail_len = 0
        self.pos = self.prompt.pos.repeat_interleave(self.fanout).contiguous()
        if alloc:
            shape = (self.L, self.B, self.kv_heads, max(self.tail_cap, 1), self.head_dim)
            self.k_tail = torch.empty(shape, dtype=BF16, device=self.device)
            self.v_tail = torch.empty(shape, dtype=BF16, device=self.device)

    def open_column(self):
        """-> the tail column the coming decode step writes (attended by construction: the tail carries no mask)"""
        if self.pos is None:
            raise ValueError("SharedPromptKVCache: begin() has not been called")
        if self.tail_len >= self.tail_cap:
            raise ValueError(f"KV cache full: {self.tail_len} of {self.tail_cap} tail columns filled")
        return self.tail_len

    def advance(self):
        self.tail_len += 1
        self.pos += 1


class LlavaHipEngine:
    supports_resid_f32 = True      # False: the subclass adds to the residual stream with bf16 primitives
    supports_ckpt = True           # False: the backward cannot re-run a layer's forward (read per pass by forward_hidden: checkpointing is ignored)
    proj_out_f32 = True            # with the fp32 stream the projector writes fp32 rows for the merge (False in a subclass: bf16)
    supports_kv_cache = True       # generate(use_cache=True): prefill into a KVCache + decode_step (vlr_decoder_layer_decode)
    row_compact_layers = True      # the adapter-free no-grad layer is vlr_decoder_layer_fwd_ex: forward_hidden(prefix_dedup=True) may run its row-compact twin

    def __init__(self, cfg: dict, device="cuda", max_positions: int = 4096):
        if not torch.cuda.is_available():
            raise _hip.VlrError("LlavaHipEngine needs an MI355X (torch.cuda.is_available() is False); "
                                "there is no CPU fallback for the DPO hot path")
        _hip.lib()
        self.cfg = dict(cfg)
        self.dev = torch.device(device)
        c = self.cfg
        self.H, self.I, self.V, self.L = c["hidden"], c["inter"], c["vocab"], c["layers"]
        self.nh = c["heads"]
        self.nkv = c.get("kv_heads") or self.nh
        self.hd = c.get("head_dim") or self.H // self.nh
        if self.hd != 128:
            raise ValueError(f"decoder head_dim must be 128 for the gfx950 attention kernels, got {self.hd}")
        if self.nh % self.nkv:
            raise ValueError(f"heads ({self.nh}) must be a multiple of kv_heads ({self.nkv})")
        self.Nq, self.Nkv = self.nh * self.hd, self.nkv * self.hd
        self.Nqkv = self.Nq + 2 * self.Nkv
        self.anyres = bool(c.get("image_grid_pinpoints"))      # LLaVA-Next tiles
        self.D = c.get("vit_hidden", 8)
        self.P = (c["image_size"] // c["patch_size"]) ** 2 if "image_size" in c else 0
        self.layout = ParamLayout(c)
        self.max_pos = max_positions
        self.cos = torch.empty(max_positions, self.hd // 2, dtype=torch.float32, device=self.dev)
        self.sin = torch.empty_like(self.cos)
        _hip.call("vlr_rope_table", self.cos, self.sin, max_positions, self.hd, float(c.get("rope_theta", 10000.0)))
        # fp32 residual stream (include/vlr.h vlr_llama_cfg.resid_f32): x0 and every layer's x_mid / x_out are fp32, never rounded.
        # Default ON (cfg["resid_f32"] = False: the bf16 stream of ABI v3); engines that compose their own layers
        # from bf16 primitives opt out (supports_resid_f32).
        self.resid_f32 = bool(c.get("resid_f32", True)) and self.supports_resid_f32
        self.RDT = torch.float32 if self.resid_f32 else BF16      # dtype of the residual stream
        # gradient checkpointing (reference scripts: --gradient_checkpointing True, dpo.py:99 non-reentrant): only the layer inputs
        # are kept by the forward; the backward re-runs each layer's forward into one scratch set right before its backward
        self.gradient_checkpointing = bool(c.get("gradient_checkpointing", False))
        self.llama_cfg = _hip.LlamaCfg(self.H, self.I, self.nh, self.hd, float(c.get("rms_eps", 1e-5)), max_positions,
                                       self.cos.data_ptr(), self.sin.data_ptr(), self.nkv, int(self.resid_f32))
        self._init_vision_cfg()
        self.vision: Optional[VisionWeights] = None
        self.policy = WeightSet(self.layout, self.dev)
        self.grads = torch.zeros(self.layout.numel, dtype=BF16, device=self.dev)
        self.gv = self.layout.views(self.grads)
        # --freeze_vision_tower False: the policy pass runs the tower of the trainable buffer, every other pass the initial one (self.vision)
        self.train_vision = "vit.patch_w" in self.layout.offset
        self.tower = TowerViews(self.policy.v, self.layout.vit_layers, _hip.VitLayerWeights) if self.train_vision else None
        self.tower_grads = TowerViews(self.gv, self.layout.vit_layers, _hip.VitLayerGrads) if self.train_vision else None
        self._vit_cache_policy = None            # _vit_cache of the trainable tower's no-grad passes; dropped at every optimizer step
        # GPTQ int4 base (q_lora): {layout entry: gptq.PackedLinear on the device} for the decoder projections, filled by load_state_dict;
        # the layer passes read a bf16 staging set that layer_weights() dequantises per call, decode_step reads the packed form itself
        self.packed = {} if c.get("gptq") else None
        self.master = self.m = self.v = None     # fp32 optimizer state, allocated by init_optimizer()
        self.opt_step = 0
        self._weights_version = 0                # bumped whenever weights are (re)loaded: keys caches derived from them
        self.vision_sd = {}
        self.grad_fresh = True                   # next backward overwrites instead of accumulating
        self._ws = {}
        self._vit_cache = None
        self.reducer = None                      # parallel.GradReducer for DDP
        self.lora = None                         # dict(r, scale, dropout) once enable_lora() ran
        self.lora_active = True                  # False inside LlavaForRL.disable_adapter() (reference pass)
        self.training = True                     # lora_dropout only in training mode
        self.neftune = None                      # dict(alpha, key) between set_neftune(alpha, ...) and set_neftune(None)
        self._neftune_calls = 0                  # noisy passes so far: the `call` word of the noise counter (checkpointed)
        self.last_neftune = None                 # (key, call, pass, T, scale) of the last noisy pass (tests replay the noise from it)
        # the reference pass computes each DPO pair's shared prompt rows once (forward_hidden(prefix_dedup=True), prefix_dedup.py)
        self.prefix_dedup = True                 # False: every pass is the dense one (the A/B switch)
        self.prefix_dedup_min_share = 1.0 / 8    # taken when the shared rows are at least this share of the M dense rows: below it the row copies cost what the GEMMs save
        self.prefix_dedup_passes = 0             # row-compact passes so far
        self.last_prefix_dedup = None            # dict(P, Mc, M) of the last row-compact pass
        # ... and so does the policy's training pass, forward and backward (forward_hidden(save=True, prefix_dedup_rows=True))
        self.prefix_dedup_policy = True          # False: the policy pass is dense (prefix_dedup = False withholds both)
        self.prefix_dedup_policy_exact_only = True   # taken only where its forward is the dense forward bit for bit (vlr_decoder_layer_compact_exact)
        self.prefix_dedup_policy_expand = False      # True: the dense backward reads expanded copies of the kept rows (vlr_layer_acts_expand) instead of the kept rows in place - the A/B of the source-row maps, same bits
        self.prefix_dedup_policy_backward = False    # True: the backward runs on the kept rows too (vlr_decoder_layer_bwd_compact): a third fewer GEMM rows, gradients within bf16 rounding of the dense backward's but not its bits
        self.prefix_dedup_policy_passes = 0      # row-compact policy passes so far
        self.last_prefix_dedup_policy = None     # dict(P, Mc, M, exact) of the last one
        self._norm_ws = torch.empty(_hip.helper("vlr_rmsnorm_bwd_workspace_bytes", self.H), dtype=torch.uint8, device=self.dev)
        self._colsum_ws = torch.empty(_hip.helper("vlr_colsum_workspace_bytes", max(self.H, self.Nqkv, 8)), dtype=torch.uint8, device=self.dev)
        self._sq_ws = torch.empty(_hip.helper("vlr_grad_sqnorm_workspace_bytes"), dtype=torch.uint8, device=self.dev)
        self._ce_ws = None                  # partials of vlr_ce_mean_fwd (allocated by the first SFT loss)
        self.ce_row_block = None            # rows per block of vlr_lmhead_ce_bwd; None = the library's default (< 1 GiB of workspace)
        self.norm_out = torch.zeros(3, dtype=torch.float32, device=self.dev)
        # split-K scratch of the GEMM dispatcher (ragged last tile rows, LoRA adapter gradients): two 64 MiB slots (main + side stream)
        _hip.ensure_splitk_workspace(self.dev, force=True)      # a new engine brings new streams: forget the old slot assignment

    # ------------------------------------------------------------------------------------------------ weights
    vision_prefix = "vision_tower."

    def _init_vision_cfg(self):
        c = self.cfg
        self.vit_cfg = _hip.VitCfg(self.D, c["vit_mlp"], c["vit_heads"], self.D // c["vit_heads"],
                                   float(c.get("vit_ln_eps", 1e-5)))
        if self.D // c["vit_heads"] != 64:
            raise ValueError("ViT head_dim must be 64 for the gfx950 attention kernels")

    def _load_vision(self, sd):
        return VisionWeights(self.cfg, sd, self.dev, prefix=self.vision_prefix + "vision_model.")

    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        if self.packed is not None:
            host = gptq.load_packed_decoder(sd, self.layout, self.cfg["gptq"]["group_size"])
            self.packed = {k: v.to(self.dev) for k, v in host.items()}
        self.policy.load_state_dict(sd)
        self.vision = self._load_vision(sd)
        # the frozen tower's ORIGINAL tensors (bf16, ~0.6 GB for CLIP-L): save_pretrained writes them back so that the
        # output directory reloads (reference trainer._save writes the whole model)
        self.vision_sd = {k: v.detach().to(device=self.dev, dtype=BF16) for k, v in sd.items() if k.startswith(self.vision_prefix)}
        self._vit_cache = None
        self._vit_cache_policy = None
        self._weights_version += 1
        if self.master is not None:
            self.init_optimizer()

    def layer_weights(self, ws: WeightSet, l, tag=None):
        """the weights of decoder layer l for ONE layer call.  Packed base: the four projections are dequantised here, on the caller's
        stream, into the bf16 staging set of pass `tag` (the reference pass runs on a side stream beside the policy pass: one set per
        tag), so call this right before the layer's forward, backward or recompute and never keep the struct."""
        v = ws.v
        bias = v[f"l{l}.bqkv"].data_ptr() if f"l{l}.bqkv" in v else None
        if self.packed is None:
            return _hip.LayerWeights(*(v[f"l{l}.{k}"].data_ptr() for k in ("ln1", "wqkv", "wo", "ln2", "wgu", "wdown")), bias)
        if tag is None:
            raise ValueError("layer_weights: a packed (GPTQ) base needs the pass tag that keys its staging set")
        st = {}
        for k in gptq.DECODER_LINEARS:
            lin = self.packed[f"l{l}.{k}"]
            st[k] = self._buf(("gptq_stage", tag, k), (lin.N, lin.K))
            _hip.call("vlr_gptq_dequant_bf16", lin.qweight, lin.qzeros, lin.scales, st[k], lin.K, lin.N, lin.g)
        return _hip.LayerWeights(v[f"l{l}.ln1"].data_ptr(), st["wqkv"].data_ptr(), st["wo"].data_ptr(), v[f"l{l}.ln2"].data_ptr(),
                                 st["wgu"].data_ptr(), st["wdown"].data_ptr(), bias)

    def layer_weights_w4(self, l):
        """the packed projections of layer l as a vlr_layer_weights_w4 (decode_step)"""
        lin = lambda k: (lambda p: _hip.W4Linear(p.qweight.data_ptr(), p.qzeros.data_ptr(), p.scales.data_ptr(), p.g))(self.packed[f"l{l}.{k}"])  # noqa: E731
        return _hip.LayerWeightsW4(*(lin(k) for k in gptq.DECODER_LINEARS))

    def packed_nbytes(self):
        """bytes of the persistent packed tensors (qweight + qzeros + scales of every decoder projection)"""
        return sum(p.nbytes() for p in self.packed.values())

    def layer_grads(self, l):
        return _hip.LayerGrads(*(self.gv[f"l{l}.{k}"].data_ptr() for k in ("ln1", "wqkv", "wo", "ln2", "wgu", "wdown")))

    # ------------------------------------------------------------------------------------------------ LoRA
    def enable_lora(self, r: int, alpha: float, dropout: float = 0.0, seed: int = 0):
        """peft get_peft_model(LoraConfig(r, lora_alpha, lora_dropout, target_modules=default_lora_target, bias='none')):
        base weights frozen, A ~ kaiming_uniform(a=sqrt(5)) = U(-1/sqrt(in), 1/sqrt(in)), B = 0.  From here on the only
        trainable parameters (gradients, optimizer state, DDP bucket) are the adapters."""
        if r <= 0 or r % 8:
            raise ValueError(f"lora_r must be a positive multiple of 8 for the gfx950 GEMM tiles, got {r}")
        if self.train_vision:
            # peft freezes every base weight, the tower included: a model laid out to train it would keep the tower's activations and run
            # its backward into gradients no optimizer reads
            raise ValueError("enable_lora on a model built with train_vision_tower: under LoRA the vision tower is frozen; load the model "
                             "without train_vision_tower")
        if self.packed is not None and not self.packed:
            raise ValueError("enable_lora on a packed (GPTQ) engine: load the checkpoint first")
        if self.Nq != self.H:
            raise NotImplementedError("LoRA needs heads * head_dim == hidden_size on the MI355X path")
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"lora_dropout must be in [0, 1), got {dropout}")
        self.lora = dict(r=int(r), scale=float(alpha) / r, dropout=float(dropout), alpha=float(alpha))
        self.lora_layout = LoraLayout(self.cfg, r)
        n = self.lora_layout.numel
        self.lora_flat = torch.zeros(n, dtype=BF16, device=self.dev)
        self.lora_grads = torch.zeros(n, dtype=BF16, device=self.dev)
        view = lambda flat: {k: flat[o: o + int(math.prod(self.lora_layout.shape[k]))].view(*self.lora_layout.shape[k])
                             for k, o in self.lora_layout.offset.items()}
        self.lv, self.lgv = view(self.lora_flat), view(self.lora_grads)
        gen = torch.Generator(device=self.dev)
        gen.manual_seed(seed)
        for k, t in self.lv.items():
            if ".a_" in k:
                bound = 1.0 / math.sqrt(t.shape[1])
                t.copy_((torch.rand(t.shape, generator=gen, device=self.dev) * 2 - 1) * bound)
            elif k.startswith(("rm_head.", "v_head.")):      # the head moves into the adapters' buffer with the values it has
                t.copy_(self.policy.v[k])
        self.lora_seed = int(seed)
        self._lora_calls = 0

        self.grads = None                         # full-parameter gradient / optimizer buffers are not needed any more
        self.gv = None
        self.master = self.m = self.v = None
        self.opt_step = 0
        self.grad_fresh = True

    def lora_state_dict(self):
        """adapter tensors under their peft adapter-file names (adapter_model.safetensors layout)"""
        out = {}
        for n, (k, lo, hi) in self.lora_layout.hf_names().items():
            t = self.lv[k][lo:hi].clone()
            perm = self.lora_layout.row_perm.get(k.split(".", 1)[1])
            if perm is not None:                  # back to the checkpoint's row order
                t = t[invert_perm(perm).to(t.device)]
            out[n] = t
        return out

    def load_lora_state_dict(self, sd):
        names = self.lora_layout.hf_names()
        norm = {k.replace(".default.weight", ".weight"): v for k, v in sd.items()}
        missing = [n for n in names if n not in norm]
        if missing:
            raise KeyError(f"missing LoRA tensors: {missing[:4]}{'...' if len(missing) > 4 else ''}")
        for n, (k, lo, hi) in names.items():
            t = norm[n]
            if tuple(t.shape) != tuple(self.lv[k][lo:hi].shape):
                raise ValueError(f"shape mismatch for {n}: {tuple(t.shape)} vs {tuple(self.lv[k][lo:hi].shape)}")
            perm = self.lora_layout.row_perm.get(k.split(".", 1)[1])
            if perm is not None:
                t = t[perm.to(t.device)]
            self.lv[k][lo:hi].copy_(t)
        if self.master is not None:
            self.init_optimizer()

    def _mask_bits(self, l, M, p, acts=None, key="lora_bits"):
        """packed lora_dropout keep masks of layer l (include/vlr.h vlr_lora_weights::mask_bits): drawn by the layer's forward, read by
        its adapter GEMMs and again by its backward - 57 MB per layer at the 7B shapes.  The buffer lives IN the activation set of the
        pass that drew it (`acts`: per tag and layer, or the one shared set of a checkpointed pass), so a second training-mode forward
        of the same size cannot overwrite masks a pending backward will read, and checkpointing keeps one buffer instead of one per
        layer.  None (no dropout, or M * width not a multiple of 32): every kernel hashes instead."""
        if p <= 0.0 or (M * self.H) % 32 or (M * self.I) % 32:
            return None
        n = _hip.helper("vlr_lora_mask_bytes", self.H, self.I, M)
        if acts is None:
            return self._buf((key, l, M), (n,), torch.uint8).data_ptr()
        sh = acts.get("shared", acts)
        t = sh.get(key)
        if t is None or t.numel() != n:
            t = sh[key] = torch.empty(n, dtype=torch.uint8, device=self.dev)
        return t.data_ptr()

    def _lora_structs(self, l, train, M=None, acts=None):
        lo = self.lora
        p = lo["dropout"] if (train and self.training) else 0.0
        ptr = lambda views, k: views[f"l{l}.{k}"].data_ptr() if f"l{l}.{k}" in views else None   # noqa: E731  (no down adapter: NULL)
        w = _hip.LoraWeights(lo["r"], lo["scale"], p, *(ptr(self.lv, k) for k in LORA_KEYS), self.lora_layout.qkv_targets,
                             self._mask_bits(l, M, p, acts) if M else None)
        g = _hip.LoraGrads(*(ptr(self.lgv, k) for k in LORA_KEYS))
        return w, g

    def merged_weights(self) -> WeightSet:
        """W + (alpha/r) B A for every adapted linear (peft merge_and_unload): a new WeightSet for export / inference."""
        if self.packed is not None:
            raise NotImplementedError("merged_weights: adapters cannot be folded into GPTQ int4 base weights (peft refuses merge_and_unload "
                                      "on a GPTQ model too); save the adapter instead")
        ws = self.policy.clone()
        r, sc = self.lora["r"], self.lora["scale"]
        for l in range(self.L):
            for g, _, targets in self.lora_layout.groups:
                W = ws.v[f"l{l}.w{g}"]
                A, B = self.lv[f"l{l}.a_{g}"], self.lv[f"l{l}.b_{g}"]
                inn = W.shape[1]
                row = 0
                for t, name in enumerate(targets):
                    out = self.lora_layout.out_dim[name]
                    Wt = W[row:row + out]
                    _hip.call("vlr_gemm_bf16_scaled", 1, B[row:row + out], A[t * r:(t + 1) * r], Wt, None, Wt,
                              out, inn, r, r, inn, inn, inn, 0, 0, 0, sc)
                    row += out
        return ws

    # ------------------------------------------------------------------------------------------------ NEFTune
    def set_neftune(self, alpha, seed=42, rank=0):
        """transformers Trainer._activate_neftune / _deactivate_neftune: alpha = neftune_noise_alpha switches the embedding noise of
        the training passes on (forward_hidden: policy weights, a pass that will be back-propagated), None switches it off.  The
        noise key is `seed` in the low word and the data-parallel `rank` in the high word, so ranks draw different noise; the call
        counter is NOT reset - a resumed run (checkpointed counter) continues the stream."""
        if alpha is None:
            self.neftune = None
            return
        alpha = float(alpha)
        if not (math.isfinite(alpha) and alpha >= 0.0):
            raise ValueError(f"neftune_noise_alpha must be a finite number >= 0, got {alpha}")
        self.neftune = dict(alpha=alpha, key=(int(seed) & 0xFFFFFFFF) | ((int(rank) & 0xFFFFFFFF) << 32))

    def _neftune_add(self, x0, src, Bn, T, S, nf):
        """x0 [Bn*S, H] (merged embeddings, either stream type) += the noise of nf = (key, call, pass, T, scale) on its text rows"""
        key, call, npass, _, scale = nf
        _hip.call("vlr_neftune_add", x0, int(x0.dtype == torch.float32), src, Bn, T, S, self.H, scale, key, call, npass)

    # ------------------------------------------------------------------------------------------------ workspaces
    def _buf(self, key, shape, dtype=BF16, zero=False):
        t = self._ws.get(key)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = (torch.zeros if zero else torch.empty)(*shape, dtype=dtype, device=self.dev)
            self._ws[key] = t
        return t

    def _layer_acts(self, tag, l, Bn, S):
        M, H, I = Bn * S, self.H, self.I
        Sp = _align(S, 64)
        k = (tag, l, Bn, S)
        t = self._ws.get(k)
        if t is None:
            t = dict(xn1=torch.empty(M, H, dtype=BF16, device=self.dev), rstd1=torch.empty(M, dtype=torch.float32, device=self.dev),
                     qkv=torch.empty(M, self.Nqkv, dtype=BF16, device=self.dev), attn=torch.empty(M, self.Nq, dtype=BF16, device=self.dev),
                     lse=torch.empty(Bn, self.nh, Sp, dtype=torch.float32, device=self.dev),
                     x_mid=torch.empty(M, H, dtype=self.RDT, device=self.dev), xn2=torch.empty(M, H, dtype=BF16, device=self.dev),
                     rstd2=torch.empty(M, dtype=torch.float32, device=self.dev), gu=torch.empty(M, 2 * I, dtype=BF16, device=self.dev),
                     act=torch.empty(M, I, dtype=BF16, device=self.dev), x_out=torch.empty(M, H, dtype=self.RDT, device=self.dev))
            t["struct"] = self._acts_struct(t)
            self._ws[k] = t
        return t

    @staticmethod
    def _acts_struct(t):
        return _hip.LayerActs(*(t[n].data_ptr() for n, _ in _hip.LayerActs._fields_))

    def _adapter_scratch(self, a, key, M, width):
        """the adapters' down-projections of one layer pass ([M][7 ranks]: `u`, or `u2` for two stacked adapters), written by the forward
        and read by the backward: lives in the activation set, or in the one shared set of a checkpointed pass"""
        sh = a.get("shared", a)
        if key not in sh or sh[key].shape[1] != width:
            sh[key] = torch.empty(M, width, dtype=BF16, device=self.dev)
        return sh[key]

    def _ckpt_acts(self, tag, l, Bn, S):
        """gradient checkpointing: every layer shares ONE scratch activation set; only x_out (= the next layer's input) is per layer"""
        k = (tag, "ckpt", l, Bn, S)
        t = self._ws.get(k)
        if t is None:
            base = self._layer_acts(tag + "/ckpt", 0, Bn, S)
            t = {n: v for n, v in base.items() if n != "struct"}
            t["x_out"] = torch.empty(Bn * S, self.H, dtype=self.RDT, device=self.dev)
            t["struct"] = self._acts_struct(t)
            t["shared"] = base            # LoRA: u / xd live in the shared set
            self._ws[k] = t
        return t

    def _norm_fwd(self, x, w, y, rstd, M):
        _hip.call("vlr_rmsnorm_fwd_f32" if x.dtype == torch.float32 else "vlr_rmsnorm_fwd", x, w, y, rstd, M, self.H, self.llama_cfg.rms_eps)

    def _norm_bwd(self, dy, x, w, rstd, dres, dx, dw, acc, M):
        _hip.call("vlr_rmsnorm_bwd_f32" if x.dtype == torch.float32 else "vlr_rmsnorm_bwd", dy, x, w, rstd, dres, dx, dw, acc, self._norm_ws, M, self.H)

    def _layer_fwd_call(self, ws, l, a, x, e, Bn, S, keep, use_lora, lora_seed):
        """one decoder layer forward into the activation set `a` (keep: also write what only the backward reads)"""
        M = Bn * S
        if use_lora:
            u = self._adapter_scratch(a, "u", M, 7 * self.lora["r"])
            lw, _ = self._lora_structs(l, train=True, M=M, acts=a)
            # (lora_dropout: the keep mask is applied to x while the adapter GEMMs stage it and regenerated in the backward - no dropped
            # copies of the seven inputs are kept any more: 0.9 GB per layer at the 7B shapes)
            _hip.call("vlr_decoder_layer_fwd_lora", self.llama_cfg, self.layer_weights(ws, l, e["tag"]), lw, a["struct"], u, None,
                      lora_seed + 8 * l, x, e["pos"], e["mask"], Bn, S)
        else:
            _hip.call("vlr_decoder_layer_fwd_ex", self.llama_cfg, self.layer_weights(ws, l, e["tag"]), a["struct"], x, e["pos"], e["mask"], Bn, S,
                      int(keep))

    # ------------------------------------------------------------------------------------------------ vision
    def vision_features(self, pixel_values: torch.Tensor, key=None, tower=None, keep=None) -> torch.Tensor:
        """CLIP ViT hidden_states[-2] without CLS -> [n*P, D] bf16 (frozen tower: cached per pixel_values tensor so the
        reference pass and the policy pass share one evaluation).  `pixel_values` may be a callable producing the [n,3,s,s]
        tensor (LLaVA-Next selects the evaluated tiles of a padded 5-D batch) - it is only called on a cache miss.
        tower (the trainable tower, self.tower): the same launches on its weights, in buffers and a cache of their own
        (_vit_cache_policy, keyed by the weights' version too).  keep (a dict, the training pass of a trainable tower): never cached;
        the pass leaves in `keep` what _vision_backward reads - the im2col patches, the patch embeddings and every layer's INPUT xs[l]
        (xs[l + 1] is layer l's output)."""
        policy = tower is not None
        if key is None:
            key = (pixel_values.data_ptr(), tuple(pixel_values.shape), pixel_values._version)
        if policy:
            key = (key, self.policy.version, self._weights_version)      # (a reload of the weights moves the tower as a step does)
        cache = self._vit_cache_policy if policy else self._vit_cache
        if keep is None and cache is not None and cache[0] == key:
            return cache[1]
        if callable(pixel_values):
            pixel_values = pixel_values()
        c = self.cfg
        n = pixel_values.shape[0]
        g = c["image_size"] // c["patch_size"]
        T = g * g + 1
        D, F = self.D, c["vit_mlp"]
        vw = tower if policy else self.vision
        # scratch per kind of pass: the reference pass may run on the side stream while the policy's training pass runs on the main one
        tag = "vit_train_" if keep is not None else ("vit_policy_" if policy else "vit_")
        pv = pixel_values.to(device=self.dev, dtype=torch.float32).contiguous()
        patches = self._buf((tag + "patches", n), (n * g * g, vw.Kp))
        _hip.call("vlr_im2col", pv, patches, n, c["image_size"], c["patch_size"], vw.Kp)
        pe = self._buf((tag + "pe", n), (n * g * g, D))
        _hip.call("vlr_gemm_bf16", 0, patches, vw.patch_w, pe, None, None, n * g * g, D, vw.Kp, vw.Kp, vw.Kp, D, 0, 0, 0, 0)
        xs = self._buf((tag + "xs", n), (len(vw.layers) + 1, n * T, D)) if keep is not None else None
        x = xs[0] if keep is not None else self._buf((tag + "x", n), (n * T, D))
        _hip.call("vlr_vit_embed_ln", pe, vw.cls, vw.pos, vw.pre_w, vw.pre_b, x, n, T, D, self.vit_cfg.ln_eps)
        wsb = dict(xn=self._buf((tag + "xn", n), (n * T, D)), qkv=self._buf((tag + "qkv", n), (n * T, 3 * D)),
                   attn=self._buf((tag + "attn", n), (n * T, D)), h=self._buf((tag + "h", n), (n * T, F)))
        ws = _hip.VitWs(*(wsb[k].data_ptr() for k in ("xn", "qkv", "attn", "h")))
        for l, lw in enumerate(vw.layers):
            if keep is not None:          # the layer runs in place: on a copy of its input, which the backward recomputes it from
                xs[l + 1].copy_(x)
                x = xs[l + 1]
            _hip.call("vlr_vit_layer_fwd", self.vit_cfg, lw, ws, x, n, T)
        rows = self._ws.get(("vit_rows", n))
        if rows is None:
            rows = (torch.arange(n * T, device=self.dev, dtype=torch.int32).view(n, T)[:, 1:]).reshape(-1).contiguous()
            self._ws[("vit_rows", n)] = rows
        feat = torch.empty(n * (T - 1), D, dtype=BF16, device=self.dev)
        _hip.call("vlr_gather_rows", x, rows, feat, n * (T - 1), D)
        if keep is not None:
            keep.update(n=n, T=T, xs=xs, pe=pe, patches=patches, rows=rows, tower=vw)
        elif policy:
            self._vit_cache_policy = (key, feat, pixel_values)
        else:
            self._vit_cache = (key, feat, pixel_values)
        return feat

    def copy_tower_from(self, vw: VisionWeights, ws: Optional[WeightSet] = None):
        """the trainable tower's tensors in `ws` (default: the policy) <- the tower `vw` (synthetic initialisers: the policy's tower
        starts as the initial one, as it does when both are loaded from one checkpoint)"""
        v = (ws or self.policy).v
        for k in ("patch_w", "cls", "pos", "pre_w", "pre_b"):
            v["vit." + k].copy_(getattr(vw, k))
        for i, t in enumerate(vw._keep):
            for k in VIT_KEYS:
                v[f"vit.l{i}.{k}"].copy_(t[k])
        self._vit_cache_policy = None

    def _vision_backward(self, ctx, vk, dz, acc):
        """d z of the projector's first linear [n_rows][H] -> the gradients of the trainable tower: d vit_feat = dz W1, scattered to the
        non-CLS rows of a zeroed [n*T][D] buffer (the inverse of the vit_rows gather), the layers top down (vlr_vit_layer_bwd recomputes
        each from its kept input), the embeddings + pre_layrnorm, and the patch kernel's d W = d patch_embeds^T patches.  The pixels get
        no gradient."""
        n, T, D, F, H = vk["n"], vk["T"], self.D, self.cfg["vit_mlp"], self.H
        M, R = n * T, n * (T - 1)
        tw, tg = vk["tower"], self.tower_grads
        dfeat = self._buf(("vit_bwd", "dfeat", n), (R, D))
        _hip.call("vlr_gemm_bf16", 1, dz, ctx["ws"].v["proj.w1"], dfeat, None, None, R, D, H, H, D, D, 0, 0, 0, 0)
        dx = self._buf(("vit_bwd", "dx", n), (M, D))
        dx.zero_()
        _hip.call("vlr_scatter_rows", dfeat, vk["rows"], dx, R, D)
        Sp = _align(T, 64)
        b = {k: self._buf(("vit_bwd", k, n), (M, w)) for k, w in (("xn1", D), ("qkv", 3 * D), ("attn", D), ("x_mid", D), ("xn2", D), ("z", F),
                                                                    ("h", F), ("dh", F), ("dxn", D), ("dqkv", 3 * D))}
        b["dattn"] = b["dxn"]
        for k in ("lse", "delta"):
            b[k] = self._buf(("vit_bwd", k, n), (n, self.vit_cfg.heads, Sp), torch.float32)
        b["norm_ws"] = self._buf(("vit_bwd", "norm_ws"), (_hip.helper("vlr_vit_layer_bwd_workspace_bytes", D, F),), torch.uint8)
        wsb = _hip.VitBwdWs(*(b[k].data_ptr() for k, _ in _hip.VitBwdWs._fields_))
        for l in range(len(tw.layers) - 1, -1, -1):
            _hip.call("vlr_vit_layer_bwd", self.vit_cfg, tw.layers[l], tg.layers[l], acc, vk["xs"][l], wsb, dx, n, T)
        dpe = self._buf(("vit_bwd", "dpe", n), (R, D))
        _hip.call("vlr_vit_embed_ln_bwd", dx, vk["pe"], tw.cls, tw.pos, tw.pre_w, dpe, tg.cls, tg.pos, tg.pre_w, tg.pre_b, acc, b["norm_ws"],
                  n, T, D, self.vit_cfg.ln_eps)
        _hip.call("vlr_gemm_bf16", 2, dpe, vk["patches"], tg.patch_w, None, None, D, tw.Kp, R, D, tw.Kp, tw.Kp, 0, 0, acc, 0)

    def anyres_vision_features(self, pixel_values, image_sizes, image_dup=1, tower=None, keep=None):
        """LLaVA-Next: the first num_patches(image_size) tiles of every DISTINCT image through the frozen ViT (cached like
        vision_features).  -> (features [tiles*P, D], sizes of the distinct images, tiles per image)"""
        from .models.LlavaNext import anyres as AR
        c = self.cfg
        if image_sizes is None:
            raise ValueError("LLaVA-Next forward needs image_sizes")
        n_img = pixel_values.shape[0]
        if n_img % image_dup:
            raise ValueError(f"{n_img} images cannot be {image_dup} identical halves")
        sizes = [tuple(int(v) for v in sz) for sz in (image_sizes.tolist() if isinstance(image_sizes, torch.Tensor) else image_sizes)]
        if len(sizes) != n_img:
            raise ValueError(f"{len(sizes)} image_sizes for {n_img} images")
        uniq = pixel_values[: n_img // image_dup]
        usz = sizes[: n_img // image_dup]
        npatch = [AR.image_size_to_num_patches(sz, c["image_grid_pinpoints"], c["image_size"]) for sz in usz]
        if uniq.dim() == 5:
            if max(npatch) > uniq.shape[1]:
                raise ValueError(f"pixel_values holds {uniq.shape[1]} tiles per image, image_sizes need {max(npatch)}")
            flat = lambda: torch.cat([uniq[i, :k] for i, k in enumerate(npatch)], dim=0)   # noqa: E731
        elif uniq.dim() == 4:
            flat = lambda: uniq                                                              # noqa: E731
        else:
            raise ValueError(f"pixel_values of shape {tuple(pixel_values.shape)}, expect to be of 4 or 5 dimensions")
        vit_feat = self.vision_features(flat, key=(pixel_values.data_ptr(), tuple(pixel_values.shape), pixel_values._version, tuple(usz)),
                                        tower=tower, keep=keep)
        if vit_feat.shape[0] != sum(npatch) * self.P:
            raise ValueError(f"{vit_feat.shape[0] // self.P} image tiles given, image_sizes need {sum(npatch)}")
        return vit_feat, usz, npatch

    def projector_fwd(self, ws: WeightSet, vit_feat, tag, extra_rows=0):
        R, H, D = vit_feat.shape[0], self.H, self.D
        z = self._buf((tag, "proj_z", R), (R, H))
        h = self._buf((tag, "proj_h", R), (R, H))
        # fp32 residual stream: the projector's output = the image rows of the merged embeddings stays fp32 (never rounded to bf16)
        f32 = self.resid_f32 and self.proj_out_f32
        out = self._buf((tag, "proj_out", R, extra_rows, f32), (R + extra_rows, H), torch.float32 if f32 else BF16)    # LLaVA-Next appends the image_newline row
        _hip.call("vlr_gemm_bf16", 0, vit_feat, ws.v["proj.w1"], z, ws.v["proj.b1"], None, R, H, D, D, D, H, 0, 0, 0, 0)
        _hip.call("vlr_gelu_fwd", z, h, z.numel())
        _hip.call("vlr_gemm_bf16", 0, h, ws.v["proj.w2"], out, ws.v["proj.b2"], None, R, H, H, H, H, H, 0, 0, 0, int(f32))
        return out, z, h

    # ------------------------------------------------------------------------------------------------ forward
    def _embed_inputs(self, ws, ids, am, lab, pixel_values, image_dup, tag, image_sizes, meta, save=False):
        """vision tower -> projector -> merge index: everything in front of the decoder.  Returns the merged-sequence geometry
        (S, src / inv maps, mask, positions, merged labels, image map) and the feature rows `feats` the merge gathers from.
        With a trainable tower the policy weights run their own tower; a pass that will be back-propagated (`save`) keeps what the
        tower's backward reads in e["vit_keep"]."""
        c = self.cfg
        Bn, T = ids.shape
        tower = self.tower if (self.train_vision and ws is self.policy) else None
        vit_keep = {} if (tower is not None and save) else None
        n_img = pixel_values.shape[0]
        if image_dup > 1:
            assert n_img % image_dup == 0
            uniq = pixel_values[: n_img // image_dup]
        else:
            uniq = pixel_values
        pack = None
        if self.anyres:
            # ---- LLaVA-Next (reference LlavaNext/__init__.py:205-265): tiles -> ViT -> projector -> anyres pack (row gather)
            from .models.LlavaNext import anyres as AR
            vit_feat, usz, npatch = self.anyres_vision_features(pixel_values, image_sizes, image_dup, tower=tower, keep=vit_keep)
            n_rows = vit_feat.shape[0]
            ext, z, h = self.projector_fwd(ws, vit_feat, tag, extra_rows=1)
            ext[n_rows].copy_(ws.v["image_newline"])
            cached = meta.get("anyres") if meta is not None else None
            if cached is None:
                pidx, lens, nl_pos = AR.pack_index(usz, npatch, c["image_grid_pinpoints"], c["image_size"], c["patch_size"])
                mi = AR.merge_index(ids.cpu().numpy(), am.cpu().numpy(), lab.cpu().numpy() if lab is not None else None,
                                    list(lens) * image_dup, int(c["image_token"]), c.get("padding_side", "left"), dup=image_dup)
                dv = lambda a_: torch.from_numpy(a_).to(self.dev)    # noqa: E731
                cached = dict(S=mi["S"], src=dv(mi["src"]), mask=dv(mi["mask"]), labels=dv(mi["labels"]), pos=dv(mi["pos"]),
                              img_map=dv(mi["img_map"]), inv=dv(mi["inv"]),
                              pack=dict(idx=dv(pidx), nl=dv(nl_pos), F=int(pidx.shape[0]), rows=n_rows, feature_lens=lens))
                if meta is not None:
                    meta["anyres"] = cached
            pack = cached["pack"]
            F = pack["F"]
            feats = self._buf((tag, "packed", F, ext.dtype), (F, self.H), ext.dtype)
            _hip.call("vlr_gather_rows", ext, pack["idx"], feats, F, self.H * (2 if ext.dtype == torch.float32 else 1))   # (row copy: fp32 rows = 2H 16-bit columns)
            S = cached["S"]
            M = Bn * S
            src, mask, pos, img_map, inv = cached["src"], cached["mask"], cached["pos"], cached["img_map"], cached["inv"]
            mlabels = cached["labels"].clone()                 # handed out as `output.labels`: every pass gets its own tensor
            n_feat = F
        else:
            vit_feat = self.vision_features(uniq, tower=tower, keep=vit_keep)
            feats, z, h = self.projector_fwd(ws, vit_feat, tag)
            n_rows = feats.shape[0]
            n_feat = n_rows
            P = self.P
            n_img_tok = (ids == c["image_token"]).sum(-1)
            if meta is not None and "S" in meta:
                S = meta["S"]
            else:
                S = int(n_img_tok.max()) * (P - 1) + T                   # one small D2H sync (shape of the merged batch)
            M = Bn * S
            src = self._buf((tag, "src", Bn, S), (Bn, S), torch.int32)
            mask = torch.empty(Bn, S, dtype=torch.int32, device=self.dev)
            mlabels = torch.empty(Bn, S, dtype=torch.int64, device=self.dev)
            pos = torch.empty(Bn, S, dtype=torch.int32, device=self.dev)
            img_map = torch.empty(Bn, S, dtype=torch.uint8, device=self.dev)
            inv = self._buf((tag, "inv", image_dup, n_rows), (image_dup, n_rows), torch.int32)
            info = torch.zeros(2, dtype=torch.int32, device=self.dev)
            _hip.call("vlr_merge_index", ids, am, lab, Bn, T, S, P, int(c["image_token"]),
                      int(c.get("model_pad_token_id", c["image_token"] + 1)), n_rows, image_dup, src, mask, mlabels, pos,
                      img_map, inv, info)
            found = n_rows * image_dup if (meta is not None and meta.get("merge_ok")) else int(info[0])   # checked once per batch
            if meta is not None:
                meta["S"], meta["merge_ok"] = S, found == n_rows * image_dup
            if found != n_rows * image_dup:
                raise ValueError(
                    f"The input provided to the model are wrong. The number of image tokens is {int(n_img_tok.sum())} while"
                    f" the number of image given to the model is {n_img}. This prevents correct indexing and breaks batch"
                    " generation.")
        return dict(S=S, M=M, src=src, mask=mask, pos=pos, labels=mlabels, img_map=img_map, inv=inv, feats=feats, vit_feat=vit_feat,
                    proj_z=z, proj_h=h, n_rows=n_rows, n_feat=n_feat, pack=pack, vit_keep=vit_keep)

    def _prefix_plan(self, e, ids, Bn, meta):
        """the row maps of a row-compact pass over this [chosen ; rejected] batch (prefix_dedup.py), or None when the shared prompt rows
        are too few to pay for the row copies.  Cached on the batch (`meta`): one small D2H read per new batch."""
        if meta is not None and "prefix_dedup" in meta:
            plan = meta["prefix_dedup"]
        else:
            S, M = e["S"], e["M"]
            src, mask, pos = (e[k].reshape(Bn, S) for k in ("src", "mask", "pos"))
            P = prefix_dedup.shared_prefix_lengths(prefix_dedup.source_key(src, ids), mask, pos).tolist()
            rows, dsrc = prefix_dedup.build_row_maps(P, S)
            twin = prefix_dedup.build_twin(rows, dsrc).to(self.dev)      # (the q|k|v epilogue stores a shared row to both of its dense rows)
            rows, dsrc = rows.to(self.dev), dsrc.to(self.dev)
            # tail: the last dense rows, all kept (the rows past the last pair's shared prefix) - vlr_decoder_layer_fwd_compact
            plan = dict(P=P, shared=sum(P), M=M, Mc=M - sum(P), tail=S - P[-1], compact_rows=rows, dense_src=dsrc, twin=twin,
                        pos=pos.reshape(-1)[rows.long()].contiguous())
            plan["struct"] = _hip.RowMaps(rows.data_ptr(), dsrc.data_ptr(), None, twin.data_ptr(), plan["pos"].data_ptr(), plan["Mc"], plan["tail"])
            if meta is not None:
                meta["prefix_dedup"] = plan
        if plan["shared"] == 0 or plan["shared"] < self.prefix_dedup_min_share * plan["M"]:
            return None
        return plan

    def _policy_plan(self, e, ids, Bn, meta):
        """the row maps of a row-compact POLICY pass over this [chosen ; rejected] batch (prefix_dedup.build_policy_plan: Mc % 8 == 0),
        on the device, or None when the pass is to run dense: too few shared rows, or - prefix_dedup_policy_exact_only - a shape at
        which the compact forward would not be the dense forward bit for bit.  Cached on the batch (`meta`) under its own key."""
        if meta is not None and "prefix_dedup_policy" in meta:
            plan = meta["prefix_dedup_policy"]
        else:
            S = e["S"]
            src, mask, pos = (e[k].reshape(Bn, S) for k in ("src", "mask", "pos"))
            if meta is not None and "prefix_dedup" in meta:
                P = meta["prefix_dedup"]["P"]                  # (the reference pass of this batch has read them already)
            else:
                P = prefix_dedup.shared_prefix_lengths(prefix_dedup.source_key(src, ids), mask, pos).tolist()
            plan = prefix_dedup.build_policy_plan(P, S)
            for k in ("compact_rows", "dense_src", "dense_own", "twin"):
                plan[k] = plan[k].to(self.dev)
            plan["pos"] = pos.reshape(-1)[plan["compact_rows"].long()].contiguous()
            plan["struct"] = _hip.RowMaps(plan["compact_rows"].data_ptr(), plan["dense_src"].data_ptr(), plan["dense_own"].data_ptr(),
                                          plan["twin"].data_ptr(), plan["pos"].data_ptr(), plan["Mc"], plan["tail"])
            if meta is not None:
                meta["prefix_dedup_policy"] = plan
        if plan["shared"] == 0 or plan["shared"] < self.prefix_dedup_min_share * plan["M"] or plan["Mc"] % 8:
            return None
        # (asked per pass: the rows the dense launches peel depend on the CUs the compute kernels have at the moment)
        plan["exact"] = bool(_hip.helper("vlr_decoder_layer_compact_exact", _hip.C.byref(self.llama_cfg), Bn, e["S"], plan["Mc"], plan["tail"]))
        if self.prefix_dedup_policy_exact_only and not plan["exact"]:
            return None
        return plan

    def _forward_layers_compact_policy(self, ws, e, plan, x0, Bn, S, tag, ckpt):
        """the decoder layers and the final norm of a pass that will be back-propagated, on the kept rows of `plan`;
        -> (hidden [M, H] dense, rstd_f [Mc], x_last [Mc], acts, x0_c [Mc]).  The activation sets are the dense pass's own (their first
        Mc rows; lse keeps its dense shape); q|k|v and the attention output also exist densely, for vlr_attn_fwd_gqa alone."""
        M, Mc, H = plan["M"], plan["Mc"], self.H
        rows, dsrc = plan["compact_rows"], plan["dense_src"]
        w16 = 2 if x0.dtype == torch.float32 else 1                  # (row copy: fp32 rows = 2H 16-bit columns)
        x0_c = self._buf((tag, "dedup_x0", Bn, S), (M, H), x0.dtype)
        _hip.call("vlr_gather_rows", x0, rows, x0_c, Mc, H * w16)
        qkv_d = self._buf((tag, "dedup_qkv", Bn, S), (M, self.Nqkv))
        attn_d = self._buf((tag, "dedup_attn", Bn, S), (M, self.Nq))
        x, acts = x0_c, []
        for l in range(self.L):
            a = self._ckpt_acts(tag, l, Bn, S) if ckpt else self._layer_acts(tag, l, Bn, S)
            self._layer_fwd_compact_call(ws, l, a, x, e, plan, qkv_d, attn_d, Bn, S, not ckpt)
            acts.append(a)
            x = a["x_out"]
        hidden_c = self._buf((tag, "dedup_hidden", Bn, S), (M, H))
        rstd_f = self._buf((tag, "rstd_f", M), (M,), torch.float32)
        self._norm_fwd(x, ws.v["norm"], hidden_c, rstd_f, Mc)
        hidden = torch.empty(M, H, dtype=BF16, device=self.dev)
        _hip.call("vlr_gather_rows", hidden_c, dsrc, hidden, M, H)
        self.prefix_dedup_policy_passes += 1
        self.last_prefix_dedup_policy = dict(P=list(plan["P"]), Mc=Mc, M=M, exact=plan["exact"], backward="compact")
        return hidden, rstd_f, x, acts, x0_c

    def _forward_layers_compact_expand(self, ws, e, plan, x0, Bn, S, tag, ckpt):
        """the decoder layers of a pass that will be back-propagated DENSELY: every layer's forward runs on the kept rows of `plan`
        into one of two scratch activation sets and what the backward reads is copied to the layer's dense set (vlr_layer_acts_expand;
        q|k|v, attn and lse are written there by the compact forward itself).  -> (x_last [M] dense, acts): the context is a dense
        pass's context, and where the plan is exact the backward computes the dense step's bits.  Under gradient checkpointing only
        x_out is copied; the recompute is the dense layer forward, as ever."""
        M, Mc, H = plan["M"], plan["Mc"], self.H
        w16 = 2 if x0.dtype == torch.float32 else 1                  # (row copy: fp32 rows = 2H 16-bit columns)
        x = self._buf((tag, "dedup_x0", Bn, S), (M, H), x0.dtype)
        _hip.call("vlr_gather_rows", x0, plan["compact_rows"], x, Mc, H * w16)
        acts = []
        for l in range(self.L):
            a = self._ckpt_acts(tag, l, Bn, S) if ckpt else self._layer_acts(tag, l, Bn, S)
            s = self._layer_acts(tag + "/compact", l % 2, Bn, S)
            sv = dict(s, lse=a["lse"])                               # the attention statistics are dense: written where the backward reads them
            self._layer_fwd_compact_call(ws, l, dict(struct=self._acts_struct(sv)), x, e, plan, a["qkv"], a["attn"], Bn, S, not ckpt)
            _hip.call("vlr_layer_acts_expand", self.llama_cfg, s["struct"], a["struct"], plan["dense_src"], M, int(not ckpt))
            acts.append(a)
            x = s["x_out"]
        self.prefix_dedup_policy_passes += 1
        self.last_prefix_dedup_policy = dict(P=list(plan["P"]), Mc=Mc, M=M, exact=plan["exact"], backward="dense")
        return acts[-1]["x_out"], acts

    def _forward_layers_compact_keep(self, ws, e, plan, x0, Bn, S, tag):
        """_forward_layers_compact_expand without the copies a row-wise consumer does not need (vlr_decoder_layer_fwd_compact_keep):
        rstd1, x_mid, rstd2, gate | up and x_out stay on the kept rows, in the first Mc rows of the layer's own activation set, and the
        backward reads them through plan["dense_src"] (vlr_decoder_layer_bwd_src); xn1, xn2 and act - the K-side operands of the
        weight-gradient GEMMs - exist densely: the norms write xn1 / xn2 to their dense rows, the fused projections read them through
        plan["compact_rows"] and the SwiGLU epilogue stores act to its dense rows (where the fused kernels take the shape; else they are copied).  The final norm runs on the kept rows and `hidden` is expanded.
        -> (hidden [M] dense, rstd_f [Mc], x_last [Mc], acts, x0_c [Mc]).  The same bits as the expand route, step for step."""
        M, Mc, H = plan["M"], plan["Mc"], self.H
        w16 = 2 if x0.dtype == torch.float32 else 1                  # (row copy: fp32 rows = 2H 16-bit columns)
        x0_c = self._buf((tag, "dedup_x0", Bn, S), (M, H), x0.dtype)
        _hip.call("vlr_gather_rows", x0, plan["compact_rows"], x0_c, Mc, H * w16)
        x, acts = x0_c, []
        for l in range(self.L):
            a = self._layer_acts(tag, l, Bn, S)
            s = self._layer_acts(tag + "/compact", l % 2, Bn, S)
            _hip.call("vlr_decoder_layer_fwd_compact_keep", self.llama_cfg, self.layer_weights(ws, l, e["tag"]), a["struct"], s["struct"], x,
                      plan["struct"], e["mask"], Bn, S)
            acts.append(a)
            x = a["x_out"]
        hidden_c = self._buf((tag, "dedup_hidden", Bn, S), (M, H))
        rstd_f = self._buf((tag, "rstd_f", M), (M,), torch.float32)
        self._norm_fwd(x, ws.v["norm"], hidden_c, rstd_f, Mc)
        hidden = torch.empty(M, H, dtype=BF16, device=self.dev)
        _hip.call("vlr_gather_rows", hidden_c, plan["dense_src"], hidden, M, H)
        self.prefix_dedup_policy_passes += 1
        self.last_prefix_dedup_policy = dict(P=list(plan["P"]), Mc=Mc, M=M, exact=plan["exact"], backward="dense")
        return hidden, rstd_f, x, acts, x0_c

    def _layer_fwd_compact_call(self, ws, l, a, x, e, plan, qkv_d, attn_d, Bn, S, keep):
        """one decoder layer forward of the row-compact policy pass into the activation set `a` (keep: also write what only the backward reads)"""
        _hip.call("vlr_decoder_layer_fwd_compact_maps", self.llama_cfg, self.layer_weights(ws, l, e["tag"]), a["struct"], x, plan["struct"],
                  qkv_d, attn_d, e["mask"], Bn, S, int(keep))

    def _forward_layers_compact(self, ws, e, plan, x0, Bn, S, tag):
        """the decoder layers and the final norm of a no-grad pass on the kept rows of `plan`; -> (hidden [M, H] dense, rstd_f, x_last)
        The activation set is the pass's dense scratch set (its first Mc rows; lse keeps its dense shape); q|k|v and the attention
        output also exist densely, for vlr_attn_fwd_gqa alone."""
        M, Mc, H = plan["M"], plan["Mc"], self.H
        rows, dsrc = plan["compact_rows"], plan["dense_src"]
        w16 = 2 if x0.dtype == torch.float32 else 1                  # (row copy: fp32 rows = 2H 16-bit columns)
        x = self._buf((tag, "dedup_x0", Bn, S), (M, H), x0.dtype)
        _hip.call("vlr_gather_rows", x0, rows, x, Mc, H * w16)
        qkv_d = self._buf((tag, "dedup_qkv", Bn, S), (M, self.Nqkv))
        attn_d = self._buf((tag, "dedup_attn", Bn, S), (M, self.Nq))
        for l in range(self.L):
            a = self._layer_acts(tag + "/scratch", l % 2, Bn, S)
            _hip.call("vlr_decoder_layer_fwd_compact_maps", self.llama_cfg, self.layer_weights(ws, l, tag), a["struct"], x, plan["struct"],
                      qkv_d, attn_d, e["mask"], Bn, S, 0)
            x = a["x_out"]
        hidden_c = self._buf((tag, "dedup_hidden", Bn, S), (M, H))
        rstd_f = self._buf((tag, "rstd_f", M), (M,), torch.float32)
        self._norm_fwd(x, ws.v["norm"], hidden_c, rstd_f, Mc)
        hidden = torch.empty(M, H, dtype=BF16, device=self.dev)
        _hip.call("vlr_gather_rows", hidden_c, dsrc, hidden, M, H)
        self.prefix_dedup_passes += 1
        self.last_prefix_dedup = dict(P=list(plan["P"]), Mc=Mc, M=M)
        return hidden, rstd_f, x

    def forward_hidden(self, ws: WeightSet, input_ids, attention_mask, labels, pixel_values, image_dup=1, save=False,
                       tag="ref", image_sizes=None, kv_cache: Optional[KVCache] = None, prefix_dedup_rows=False):
        """embed -> ViT -> projector -> merge -> decoder -> final RMSNorm.  Returns a context dict with the final
        hidden states [Bn*S, H] and the merged labels / mask / positions.  kv_cache (generate's prefill, no-grad, engines with
        supports_kv_cache): each layer's post-RoPE K / V rows are copied into it right after the layer ran.
        prefix_dedup_rows (the trainer's reference passes): a no-grad pass over a [chosen ; rejected] batch (image_dup == 2) computes the
        rows of each pair's shared prompt once (_prefix_plan) - the context keeps its dense contract, ctx["x_last"] alone is compact.
        With save=True on the policy weights (the DPO trainer's policy pass) the training forward does the same (_policy_plan: full
        fine-tune, no NEFTune; by default only where the compact forward is the dense one bit for bit) and copies what the backward
        reads to the dense layout: the context is a dense pass's.  Without gradient checkpointing (and unless prefix_dedup_policy_expand)
        only act is copied (xn1 / xn2 are written densely) and the dense backward reads the rest at dense_src[row]: ctx["src_plan"] is set, ctx["plan"]
        stays None, the layers' rstd1 / x_mid / rstd2 / gu / x_out, ctx["x_last"], ctx["rstd_f"] and ctx["x0_c"] hold the kept rows,
        ctx["hidden"] is dense.  With prefix_dedup_policy_backward the backward runs on the kept rows
        too: ctx["plan"] is set, ctx["acts"], ctx["x_last"], ctx["rstd_f"] and ctx["x0_c"] hold the kept rows, ctx["hidden"] is dense."""
        c = self.cfg
        if ws is self.policy:
            self.wait_optimizer()
        Bn, T = input_ids.shape
        meta = getattr(input_ids, "_vlr_meta", None)      # per-batch cache of host-side integers (None: always recompute)
        ids = input_ids.to(self.dev).contiguous()
        am = attention_mask.to(self.dev).contiguous()
        lab = labels.to(self.dev).contiguous() if labels is not None else None
        if self.train_vision:
            e = self._embed_inputs(ws, ids, am, lab, pixel_values, image_dup, tag, image_sizes, meta, save=bool(save))
        else:
            e = self._embed_inputs(ws, ids, am, lab, pixel_values, image_dup, tag, image_sizes, meta)
        e["tag"] = tag               # scratch buffers of layers composed in Python are keyed per pass (the reference pass runs on a side stream)
        e["grad_pass"] = bool(save)  # this pass will be back-propagated (training-mode dropout applies; a checkpointed forward included)
        S, M = e["S"], e["M"]
        src, mask, pos, mlabels, img_map, inv = e["src"], e["mask"], e["pos"], e["labels"], e["img_map"], e["inv"]
        if kv_cache is not None:
            if save or not self.supports_kv_cache:
                raise ValueError("forward_hidden: kv_cache needs a no-grad pass of an engine with supports_kv_cache")
            kv_cache.reserve(S)
        feats, vit_feat, z, h, n_rows, n_feat, pack = e["feats"], e["vit_feat"], e["proj_z"], e["proj_h"], e["n_rows"], e["n_feat"], e["pack"]
        if self.resid_f32:                 # fp32 stream: embedding rows widened exactly, the projector's output rows unrounded (fp32 feats)
            x0 = self._buf((tag, "x0f", Bn, S), (M, self.H), torch.float32)
            _hip.call("vlr_merge_fwd_f32", src, ids, ws.v["embed"], feats, int(feats.dtype == torch.float32), x0, Bn, T, S, self.H)
        else:
            x0 = self._buf((tag, "x0", Bn, S), (M, self.H))
            _hip.call("vlr_merge_fwd", src, ids, ws.v["embed"], feats, x0, Bn, T, S, self.H)
        # NEFTune: noise on the text rows of a TRAINING pass only (the condition of training-mode dropout: policy weights, a pass that
        # will be back-propagated).  Reference passes - a separate reference model, the adapter-off pass, precomputed or prefetched
        # reference log-probs - evaluation and generation never come here.  One draw per pass: under gradient checkpointing the
        # recompute reads this x0 (ctx["x0"]).  NO path rebuilds x0 today; ctx["neftune"] (the draw's key - nothing but the tests reads
        # it) is what such a path would have to reuse instead of bumping the counter.
        nf = None
        if self.neftune is not None and ws is self.policy and save:
            self._neftune_calls += 1
            nf = (self.neftune["key"], self._neftune_calls & 0xFFFFFFFF, 0, T, neftune_scale(self.neftune["alpha"], T, self.H)[1])
            self._neftune_add(x0, src, Bn, T, S, nf)
            self.last_neftune = nf
        x = x0
        acts = []
        use_lora = self.lora is not None and self.lora_active and ws is self.policy
        lora_seed = None
        if use_lora:
            self._lora_calls += 1
            lora_seed = (self.lora_seed << 40) + (self._lora_calls << 16)        # + 8*layer + target inside the library
        ckpt = bool(save and self.gradient_checkpointing and self.supports_ckpt)      # (layers composed in Python keep their activations)
        plan = None
        if (prefix_dedup_rows and self.prefix_dedup and self.row_compact_layers and not save and kv_cache is None and image_dup == 2
                and not use_lora and Bn % 2 == 0):
            plan = self._prefix_plan(e, ids, Bn, meta)
        # the policy's training pass (VLDPOTrainer asks for it): the forward on the kept rows, the backward dense on the expanded
        # activations (the dense step's bits where the plan is exact) or - prefix_dedup_policy_backward - on the kept rows too (one more
        # bf16 rounding per shared d qkv row).  NEFTune draws different noise for the two copies of a prompt row: under it the rows are
        # not equal, and the pass is dense
        pplan, x0_c, layers_done, src_plan = None, None, False, None
        if (prefix_dedup_rows and self.prefix_dedup and self.prefix_dedup_policy and self.row_compact_layers and save and ws is self.policy
                and kv_cache is None and image_dup == 2 and not use_lora and self.lora is None and Bn % 2 == 0 and self.neftune is None):
            pplan = self._policy_plan(e, ids, Bn, meta)
        if plan is not None:
            hidden, rstd_f, x = self._forward_layers_compact(ws, e, plan, x0, Bn, S, tag)
        elif pplan is not None and self.prefix_dedup_policy_backward:
            hidden, rstd_f, x, acts, x0_c = self._forward_layers_compact_policy(ws, e, pplan, x0, Bn, S, tag, ckpt)
            plan = pplan
        elif pplan is not None and not ckpt and not self.prefix_dedup_policy_expand:
            # compact forward, dense backward reading the kept rows in place: ctx["src_plan"] (NOT ctx["plan"]: the backward is dense);
            # acts hold rstd / x_mid / gate|up / x_out on the kept rows, x_last, rstd_f and x0_c too; hidden is dense
            hidden, rstd_f, x, acts, x0_c = self._forward_layers_compact_keep(ws, e, pplan, x0, Bn, S, tag)
            src_plan, pplan, layers_done = pplan, None, True
        elif pplan is not None:         # compact forward, dense backward: the context below is a dense pass's (the final norm runs on M rows)
            x, acts = self._forward_layers_compact_expand(ws, e, pplan, x0, Bn, S, tag, ckpt)
            pplan, layers_done = None, True
        for l in range(self.L if plan is None and not layers_done else 0):
            if ckpt:
                a = self._ckpt_acts(tag, l, Bn, S)
            else:
                a = self._layer_acts(tag if save else tag + "/scratch", l if save else (l % 2), Bn, S)   # scratch per pass tag (side stream)
            # checkpointing: this pass keeps x_out only - what the backward reads is written by the recompute (hidden_backward)
            self._layer_fwd_call(ws, l, a, x, e, Bn, S, save and not ckpt, use_lora, lora_seed)
            if kv_cache is not None:      # (the scratch activation sets alternate per layer: the K / V columns are taken now)
                qkv = a["qkv"]
                _hip.call("vlr_kv_cache_write", qkv[:, self.Nq:], qkv[:, self.Nq + self.Nkv:], self.Nqkv, kv_cache.k[l], kv_cache.v[l],
                          Bn, S, self.nkv, self.hd, kv_cache.cap, 0)
            acts.append(a)
            x = a["x_out"]
        if plan is None and src_plan is None:
            hidden = torch.empty(M, self.H, dtype=BF16, device=self.dev)
            rstd_f = self._buf((tag, "rstd_f", M), (M,), torch.float32)
            self._norm_fwd(x, ws.v["norm"], hidden, rstd_f, M)
        if kv_cache is not None:
            kv_cache.start(mask.view(Bn, S))
        return dict(ws=ws, Bn=Bn, T=T, S=S, M=M, ids=ids, src=src, inv=inv, mask=mask, labels=mlabels, pos=pos,
                    img_map=img_map.bool(), hidden=hidden, rstd_f=rstd_f, x_last=x, x0=x0, acts=acts if save else None,
                    vit_feat=vit_feat, feats=feats, proj_z=z, proj_h=h, image_dup=image_dup, n_rows=n_rows, n_feat=n_feat,
                    pack=pack, tag=tag, lora_seed=lora_seed, neftune=nf, meta=meta, extra=e.get("extra"), ckpt=ckpt, use_lora=use_lora,
                    plan=pplan, x0_c=x0_c,     # a row-compact policy pass: acts, x_last, rstd_f and x0_c hold the plan's Mc kept rows; hidden is dense
                    vit_keep=e.get("vit_keep"),   # a trainable tower's training pass: what _vision_backward reads
                    src_plan=src_plan,         # a dense backward that reads the kept rows in place (_forward_layers_compact_keep)
                    embed=dict(pos=e["pos"], mask=e["mask"], extra=e.get("extra"), tag=tag, img_map=e["img_map"], plora_seed=e.get("plora_seed"), grad_pass=bool(save)))

    # ------------------------------------------------------------------------------------------------ decoding
    def new_kv_cache(self, batch, new_tokens) -> KVCache:
        """an empty cache for `batch` sequences and `new_tokens` decode columns; the prefill (forward_hidden(kv_cache=...)) sizes it"""
        cache = KVCache(self.L, batch, self.nkv, self.hd, new_tokens, self.dev)
        cache.position_rule = self.kv_next_positions
        return cache

    @staticmethod
    def kv_next_positions(key_mask, length=None):
        """[B] int32: the rotary position of the token each row appends after a prefill of `length` columns.  The engine's rule, consulted
        by KVCache.start (and through the prompt cache by SharedPromptKVCache.begin): here the merge's - the number of attended columns."""
        return KVCache.next_positions(key_mask, length)

    wide_gemv = True               # batches above 16 rows take the skinny GEMMs 64 rows per weight pass (False: 16-row groups; same bits)
    wide_gemv_w4 = True            # ... over packed int4 weights too (vlr_gemv_wide_w4); wide_gemv = False withholds both

    def _gemv_rows(self, mode, X, W, Y, M, N, K, ws):
        """the lm-head of a decode step: 16 rows per call, or - above 16 rows, `ws` sized for it by _decode_ws - 64 (vlr_gemv_wide_bf16)"""
        wide = M > 16 and self.wide_gemv and ws.numel() >= int(_hip.lib().vlr_gemv_wide_workspace_bytes(min(M, 64), N, K))
        fn, rows = ("vlr_gemv_wide_bf16", 64) if wide else ("vlr_gemv_bf16", 16)
        for m0 in range(0, M, rows):
            mr = min(rows, M - m0)
            _hip.call(fn, mode, X[m0:m0 + mr], X.shape[1], W, Y[m0:m0 + mr], Y.shape[1], None, None, 0, None, None, None,
                      0, self.hd, self.max_pos, mr, N, K, ws)

    def new_shared_kv_cache(self, prompts, fanout, new_tokens) -> SharedPromptKVCache:
        """an empty shared-prompt cache: prefill `cache.prompt` (forward_hidden(kv_cache=cache.prompt)), then cache.begin()"""
        cache = SharedPromptKVCache(self.L, prompts, fanout, self.nkv, self.hd, new_tokens, self.dev)
        cache.prompt.position_rule = self.kv_next_positions
        return cache

    def _decode_ws(self, B, cap, shared=None):
        """shared: (prompts, fanout, prompt_cap, tail_cap) of a SharedPromptKVCache - sizes the attention workspace for it"""
        key = ("decode_ws", B, cap, self.lora["r"] if self.lora is not None else 0, shared, bool(self.wide_gemv), bool(getattr(self, "wide_gemv_w4", False)))
        d = self._ws.get(key)
        if d is None:
            self._ws = {k: v for k, v in self._ws.items() if not (isinstance(k, tuple) and k and k[0] == "decode_ws")}
            mb = min(B, 16)
            shapes = ((self.Nqkv, self.H), (self.H, self.Nq), (2 * self.I, self.H), (self.H, self.I), (self.V, self.H))
            gb = max(int(_hip.lib().vlr_gemv_workspace_bytes(mb, n, k)) for n, k in shapes)
            if self.packed is not None:      # the packed skinny GEMM splits K differently
                gb = max([gb] + [int(_hip.lib().vlr_gemv_w4_workspace_bytes(mb, n, k)) for n, k in shapes[:4]])
            ub = 0
            if self.lora is not None:        # live adapters (decode_step on the policy): one more partial slice, and the x A^T partials
                r = self.lora["r"]
                nq = self.lora_layout.qkv_targets
                rt = (nq * r, r, 2 * r, r)
                gb = max([gb] + [int(_hip.lib().vlr_gemv_lora_workspace_bytes(mb, n, k, t)) for (n, k), t in zip(shapes[:4], rt)])
                ub = max(int(_hip.lib().vlr_gemv_lora_u_bytes(mb, k, t)) for (n, k), t in zip(shapes[:4], rt))
            if B > 16 and self.wide_gemv and (self.packed is None or getattr(self, "wide_gemv_w4", False)):
                # scratch for 64-row groups - what makes vlr_decoder_layer_decode* and the lm-head (bf16 in a packed model too) take the
                # wide calls
                mw = min(B, 64)
                gb = max([gb] + [int(_hip.lib().vlr_gemv_wide_workspace_bytes(mw, n, k)) for n, k in shapes])
                if self.packed is not None:
                    gb = max([gb] + [int(_hip.lib().vlr_gemv_wide_w4_workspace_bytes(mw, n, k)) for n, k in shapes[:4]])
                if self.lora is not None:
                    gb = max([gb] + [int(_hip.lib().vlr_gemv_wide_lora_workspace_bytes(mw, n, k, t)) for (n, k), t in zip(shapes[:4], rt)])
                    ub = max([ub] + [int(_hip.lib().vlr_gemv_wide_lora_u_bytes(mw, k, t)) for (n, k), t in zip(shapes[:4], rt)])
            if shared is not None:
                ab = int(_hip.lib().vlr_attn_decode_shared_workspace_bytes(shared[0], shared[1], self.nh, shared[2], shared[3]))
            else:
                ab = int(_hip.lib().vlr_attn_decode_workspace_bytes(B, self.nh, cap))
            d = dict(xn=torch.empty(B, self.H, dtype=BF16, device=self.dev), rstd=torch.empty(B, dtype=torch.float32, device=self.dev),
                     qkv=torch.empty(B, self.Nqkv, dtype=BF16, device=self.dev), attn=torch.empty(B, self.Nq, dtype=BF16, device=self.dev),
                     act=torch.empty(B, self.I, dtype=BF16, device=self.dev), gemv=torch.empty(gb, dtype=torch.uint8, device=self.dev),
                     attn_ws=torch.empty(ab, dtype=torch.uint8, device=self.dev), x=torch.empty(B, self.H, dtype=self.RDT, device=self.dev),
                     xe=torch.empty(B, self.H, dtype=BF16, device=self.dev), hidden=torch.empty(B, self.H, dtype=BF16, device=self.dev))
            d["struct"] = _hip.DecodeWs(d["xn"].data_ptr(), d["rstd"].data_ptr(), d["qkv"].data_ptr(), d["attn"].data_ptr(),
                                        d["act"].data_ptr(), d["gemv"].data_ptr(), gb, d["attn_ws"].data_ptr(), ab)
            if ub:
                d["u"] = torch.empty(ub, dtype=torch.uint8, device=self.dev)
                d["lora_struct"] = _hip.DecodeLoraWs(d["u"].data_ptr(), ub)
            self._ws[key] = d
        return d

    def decode_step(self, ws: WeightSet, tokens, cache: KVCache, lora=None):
        """One new token per sequence against the cache (transformers LlamaModel.forward with a DynamicCache, one query row):
        embedding row gather -> L x vlr_decoder_layer_decode -> final RMSNorm -> lm-head (skinny GEMM, fp32 out).
        tokens [B] (ids appended at column cache.len) -> logits fp32 [B][V]; the cache advances by one column.
        lora (None: forward_hidden's rule - the adapters are live when `ws` is the policy and they are active; False: never): live
        adapters run vlr_decoder_layer_decode_lora / _w4_lora, un-merged; everything else makes the adapter-free calls.
        cache: a KVCache, or a SharedPromptKVCache (B = prompts * fanout rows: every layer is one vlr_decoder_layer_decode_shared, which
        takes the same three weight routes)."""
        if not self.supports_kv_cache:
            raise ValueError(f"{type(self).__name__} has no KV-cache decoding")
        B, H = cache.B, self.H
        use_lora = self.lora is not None and self.lora_active and ws is self.policy
        if lora is not None:
            if lora and not use_lora:
                raise ValueError("decode_step(lora=True): live adapters need the policy weights and active adapters")
            use_lora = bool(lora)
        shared = isinstance(cache, SharedPromptKVCache)
        if shared:
            d = self._decode_ws(B, cache.cap, (cache.P, cache.fanout, cache.prompt.cap, cache.tail_cap))
        else:
            d = self._decode_ws(B, cache.cap)
        tok = tokens.to(device=self.dev, dtype=torch.int32).contiguous()
        length = cache.open_column()
        x = d["x"]
        if self.resid_f32:                 # the embedding rows widened exactly (vlr_merge_fwd_f32's rule)
            _hip.call("vlr_gather_rows", ws.v["embed"], tok, d["xe"], B, H)
            _hip.call("vlr_cast_bf16_to_f32", d["xe"], x, B * H)
        else:
            _hip.call("vlr_gather_rows", ws.v["embed"], tok, x, B, H)
        for l in range(self.L):
            if shared:
                pr = cache.prompt
                kv = _hip.KvShared(pr.k[l].data_ptr(), pr.v[l].data_ptr(), pr.key_mask.data_ptr(), cache.P, pr.cap, pr.len,
                                   cache.k_tail[l].data_ptr(), cache.v_tail[l].data_ptr(), cache.fanout, cache.tail_cap, length + 1)
                if self.packed is not None:
                    v = ws.v
                    w = _hip.LayerWeights(v[f"l{l}.ln1"].data_ptr(), None, None, v[f"l{l}.ln2"].data_ptr(), None, None,
                                          v[f"l{l}.bqkv"].data_ptr() if f"l{l}.bqkv" in v else None)
                    q4 = self.layer_weights_w4(l)
                else:
                    w, q4 = self.layer_weights(ws, l), None
                _hip.call("vlr_decoder_layer_decode_shared", self.llama_cfg, w, q4, self._lora_structs(l, train=False)[0] if use_lora else None,
                          d["struct"], d["lora_struct"] if use_lora else None, x, cache.pos, kv)
                continue
            if self.packed is not None:      # the projections stream their 4-bit form: nothing is dequantised to HBM
                v = ws.v
                w = _hip.LayerWeights(v[f"l{l}.ln1"].data_ptr(), None, None, v[f"l{l}.ln2"].data_ptr(), None, None,
                                      v[f"l{l}.bqkv"].data_ptr() if f"l{l}.bqkv" in v else None)
                if use_lora:
                    _hip.call("vlr_decoder_layer_decode_w4_lora", self.llama_cfg, w, self.layer_weights_w4(l), self._lora_structs(l, train=False)[0],
                              d["struct"], d["lora_struct"], x, cache.pos, cache.k[l], cache.v[l], cache.key_mask, B, cache.cap, length)
                    continue
                _hip.call("vlr_decoder_layer_decode_w4", self.llama_cfg, w, self.layer_weights_w4(l), d["struct"], x, cache.pos, cache.k[l],
                          cache.v[l], cache.key_mask, B, cache.cap, length)
                continue
            if use_lora:
                _hip.call("vlr_decoder_layer_decode_lora", self.llama_cfg, self.layer_weights(ws, l), self._lora_structs(l, train=False)[0],
                          d["struct"], d["lora_struct"], x, cache.pos, cache.k[l], cache.v[l], cache.key_mask, B, cache.cap, length)
                continue
            _hip.call("vlr_decoder_layer_decode", self.llama_cfg, self.layer_weights(ws, l), d["struct"], x, cache.pos, cache.k[l],
                      cache.v[l], cache.key_mask, B, cache.cap, length)
        self._norm_fwd(x, ws.v["norm"], d["hidden"], d["rstd"], B)
        logits = torch.empty(B, self.V, dtype=torch.float32, device=self.dev)
        self._gemv_rows(_hip.GEMV_F32, d["hidden"], ws.v["lm_head"], logits, B, self.V, H, d["gemv"])
        cache.advance()
        return logits

    # ------------------------------------------------------------------------------------------------ log-probs
    def logps_forward(self, ctx, labels, shared_mask=None, average=False, label_pad=-100, reduce_seq=True, entropy=False):
        """get_batch_logps on the lm-head restricted to the response rows (identical result: every other row is
        multiplied by a zero mask in the reference, base/trainer.py:185-188).  Returns (logps [Bn], lp_ctx).  entropy: the lm-head pass
        with the row entropy (vlr_lmhead_logps_entropy_fwd: the same log-probs bit for bit) -> lp_ctx["entropy"] [R]."""
        Bn, S, M, H, V = ctx["Bn"], ctx["S"], ctx["M"], self.H, self.V
        ws = ctx["ws"]
        if tuple(labels.shape) != (Bn, S):
            raise ValueError("Logits (batch and sequence length dim) and labels must have the same shape.")
        lab = labels.to(self.dev).contiguous()
        rows = torch.empty(M, dtype=torch.int32, device=self.dev)
        tgt = torch.empty(M, dtype=torch.int32, device=self.dev)
        seq_off = torch.empty(Bn + 1, dtype=torch.int32, device=self.dev)
        sm = shared_mask.to(device=self.dev, dtype=torch.uint8).contiguous() if shared_mask is not None else None
        _hip.call("vlr_build_rows", lab, sm, Bn, S, label_pad, rows, tgt, seq_off)
        meta, rkey = ctx.get("meta"), ("R" if reduce_seq else "R_ce", sm is not None, int(label_pad))      # (the SFT mask is not the DDPO mask)
        if meta is not None and rkey in meta:
            R = meta[rkey]
        else:
            R = int(seq_off[-1])                                      # one small D2H sync (row count of the lm-head GEMM)
            if meta is not None:
                meta[rkey] = R
        logps = torch.zeros(Bn, dtype=torch.float32, device=self.dev)
        lp = dict(R=R, rows=rows, tgt=tgt, seq_off=seq_off, average=average, ctx=ctx)
        if R == 0:
            return logps, lp
        hg = torch.empty(R, H, dtype=BF16, device=self.dev)
        _hip.call("vlr_gather_rows", ctx["hidden"], rows, hg, R, H)
        # fused lm-head + log-softmax pick: at the 7B shapes the [R][V] logits never reach HBM (include/vlr.h); small shapes go
        # through an fp32 logits buffer (per pass tag: the reference pass runs on a side stream)
        fused = bool(_hip.helper("vlr_lmhead_is_fused", R, V, H))
        lws = self._buf(("lmhead_ws", ctx["tag"], R), (int(_hip.lib().vlr_lmhead_workspace_bytes(R, V)),), torch.uint8)
        logits = None if fused else self._buf(("logits", ctx["tag"], R), (R, V), torch.float32)
        tok = torch.empty(R, dtype=torch.float32, device=self.dev)
        lse = torch.empty(R, dtype=torch.float32, device=self.dev)
        if entropy:
            ews = self._buf(("lmhead_ent_ws", ctx["tag"], R), (int(_hip.lib().vlr_lmhead_entropy_workspace_bytes(R, V)),), torch.uint8)
            ent = torch.empty(R, dtype=torch.float32, device=self.dev)
            _hip.call("vlr_lmhead_logps_entropy_fwd", hg, ws.v["lm_head"], tgt, tok, lse, ent, ews, logits, R, V, H)
            lp["entropy"] = ent
        else:
            _hip.call("vlr_lmhead_logps_fwd", hg, ws.v["lm_head"], tgt, tok, lse, lws, logits, R, V, H)
        if reduce_seq:
            _hip.call("vlr_seq_sum", tok, seq_off, Bn, int(average), logps)
        lp.update(hg=hg, lse=lse, tok=tok)
        return logps, lp

    def ce_forward(self, ctx, labels, shift_mask=None, label_pad=-100):
        """The causal-LM cross-entropy of the reference wrappers' forward(labels=...): mean of -log p(label) over the rows of the WHOLE
        batch whose shifted label is not `label_pad` (and whose shifted `shift_mask` [Bn, S-1] is non-zero, when given: the LLaVA
        wrappers select by the merged attention mask).  The rows go through the same fused lm-head as the log-probs; vlr_ce_mean_fwd
        folds them in a fixed order.  Returns (out3 = {loss, row count, -1 / rows} on the device, lp_ctx)."""
        _, lp = self.logps_forward(ctx, labels, shift_mask, False, label_pad, reduce_seq=False)
        out3 = torch.empty(3, dtype=torch.float32, device=self.dev)
        if lp["R"] == 0:                      # nn.CrossEntropyLoss over no row: nan
            out3.copy_(torch.tensor([float("nan"), 0.0, 0.0]))
            return out3, lp
        if self._ce_ws is None:
            self._ce_ws = torch.empty(_hip.helper("vlr_ce_mean_workspace_bytes"), dtype=torch.uint8, device=self.dev)
        _hip.call("vlr_ce_mean_fwd", lp["tok"], lp["R"], self._ce_ws, out3)
        lp["out3"] = out3
        return out3, lp

    def ce_backward(self, lp, dloss, row_block=None):
        """d loss (scalar) -> d hidden (dense [M,H], zero outside the label rows) and the lm_head weight gradient, the rows walked in
        blocks (vlr_lmhead_ce_bwd): d logits exists for `row_block` rows at a time (default: under 1 GiB of workspace)."""
        ctx = lp["ctx"]
        M, H, V, R = ctx["M"], self.H, self.V, lp["R"]
        acc = int(not self.grad_fresh)
        dhidden = torch.zeros(M, H, dtype=BF16, device=self.dev)
        if R == 0:
            if not acc and self.lora is None:
                self.gv["lm_head"].zero_()
            return dhidden
        rb = int(row_block if row_block else (self.ce_row_block or _hip.helper("vlr_lmhead_ce_row_block", R, V, H)))
        rb = min(rb, R)
        sizes = {rb} | ({R % rb} if R % rb else set())
        loose = [n for n in sizes if not _hip.helper("vlr_lmhead_is_fused", n, V, H)]
        lws = self._buf(("lmhead_ws", ctx["tag"], rb), (int(_hip.lib().vlr_lmhead_workspace_bytes(rb, V)),), torch.uint8)
        logits = self._buf(("logits", ctx["tag"], max(loose)), (max(loose), V), torch.float32) if loose else None
        dl = self._buf(("dlogits", rb), (rb, V))
        coef = (dloss.to(torch.float32).reshape(1) * lp["out3"][2:3]).contiguous()
        dhg = torch.empty(R, H, dtype=BF16, device=self.dev)
        _hip.call("vlr_lmhead_ce_bwd", lp["hg"], ctx["ws"].v["lm_head"], lp["tgt"], lp["lse"], coef, dl, lws, logits, dhg,
                  self.gv["lm_head"] if self.lora is None else None, acc, R, V, H, rb)      # under LoRA the lm_head is frozen
        _hip.call("vlr_scatter_rows", dhg, lp["rows"], dhidden, R, H)
        if self.reducer is not None and self.lora is None:
            self.reducer.bucket_ready("lm_head")
        return dhidden

    # ------------------------------------------------------------------------------------------------ reward head
    def rm_head_views(self):
        """(weight [H], bias [1], d weight, d bias) of the reward head in the trainable buffers of the mode in use"""
        if not self.cfg.get("rm_head"):
            raise ValueError("this engine was built without cfg['rm_head']: it has no reward head")
        if self.lora is not None:
            return self.lv["rm_head.w"], self.lv["rm_head.b"], self.lgv["rm_head.w"], self.lgv["rm_head.b"]
        return self.policy.v["rm_head.w"], self.policy.v["rm_head.b"], self.gv["rm_head.w"], self.gv["rm_head.b"]

    def set_rm_head(self, weight, bias):
        """loads the head (rm_head.bin: weight [1, H] or [H], bias [1]); the optimizer's master copy follows"""
        w, b, _, _ = self.rm_head_views()
        w.copy_(weight.reshape(-1).to(device=self.dev, dtype=BF16))
        b.copy_(bias.reshape(-1).to(device=self.dev, dtype=BF16))
        self._weights_version += 1
        if self.master is not None:
            self.init_optimizer()

    def reward_forward(self, ctx, rows):
        """rewards[i] = rm_head(hidden[rows[i]]) in fp32 (vlr_rm_head_fwd); rows: dense row indices b * S + column into the final hidden
        states of `ctx`, one per sequence.  The lm-head never runs.  Returns (rewards [n] fp32, rw_ctx)."""
        w, b, _, _ = self.rm_head_views()
        rows = rows.to(device=self.dev, dtype=torch.int32).contiguous()
        n = rows.numel()
        rewards = torch.empty(n, dtype=torch.float32, device=self.dev)
        _hip.call("vlr_rm_head_fwd", ctx["hidden"], self.H, rows, w, b, rewards, n, self.H)
        return rewards, dict(ctx=ctx, rows=rows, n=n)

    def reward_backward(self, lp, d_rewards):
        """d rewards -> d hidden (dense [M,H], zero outside the reward rows) and the head's gradients (vlr_rm_head_bwd).  The lm-head
        takes part in the reference's graph with a zero gradient (0.0 * mean(logits)): in a full fine-tune its gradient stays zero -
        zeroed here on a fresh gradient buffer, as logps_backward does for R == 0."""
        ctx = lp["ctx"]
        w, _, gw, gb = self.rm_head_views()
        acc = int(not self.grad_fresh)
        dhidden = torch.zeros(ctx["M"], self.H, dtype=BF16, device=self.dev)
        _hip.call("vlr_rm_head_bwd", ctx["hidden"], self.H, lp["rows"], w, d_rewards.to(torch.float32).contiguous(), dhidden, self.H,
                  gw, gb, acc, lp["n"], self.H)
        if self.lora is None:
            if not acc:
                self.gv["lm_head"].zero_()
            if self.reducer is not None:
                self.reducer.bucket_ready("lm_head")
        return dhidden

    # ------------------------------------------------------------------------------------------------ PPO: value head + per-token heads
    def v_head_views(self):
        """(weight [H], bias [1], d weight, d bias) of the PPO value head in the trainable buffers of the mode in use"""
        if not self.cfg.get("v_head"):
            raise ValueError("this engine was built without cfg['v_head']: it has no value head")
        if self.lora is not None:
            return self.lv["v_head.w"], self.lv["v_head.b"], self.lgv["v_head.w"], self.lgv["v_head.b"]
        return self.policy.v["v_head.w"], self.policy.v["v_head.b"], self.gv["v_head.w"], self.gv["v_head.b"]

    def set_v_head(self, weight, bias):
        """loads the head (v_head.summary.weight [1, H] or [H], v_head.summary.bias [1]); the optimizer's master copy follows"""
        w, b, _, _ = self.v_head_views()
        w.copy_(weight.reshape(-1).to(device=self.dev, dtype=BF16))
        b.copy_(bias.reshape(-1).to(device=self.dev, dtype=BF16))
        self._weights_version += 1
        if self.master is not None:
            self.init_optimizer()

    def _row_range(self, n):
        """0..n-1 as int32 on the device (the value head reads every gathered row; every row its own sequence in the lm-head backward)"""
        t = self._ws.get(("row_range",))
        if t is None or t.numel() < n:
            t = self._ws[("row_range",)] = torch.arange(max(n, 4096), dtype=torch.int32, device=self.dev)
        return t[:n]

    def token_logps_forward(self, ctx, labels, label_pad=-100, entropy=False):
        """per-token log-probs on the R response rows (the rows whose logits predict a label != label_pad): the fused lm-head of
        logps_forward(reduce_seq=False).  Needs no value head.  Returns (tok_logp [R] fp32, lp_ctx); lp_ctx["seq_off"] delimits the
        sequences.  entropy: lp_ctx["entropy"] [R] fp32 beside lp_ctx["tok"], from the same lm-head pass; the log-probs keep their bits."""
        _, lp = self.logps_forward(ctx, labels, None, False, label_pad, reduce_seq=False, entropy=entropy)
        if lp["R"] == 0:
            raise ValueError("token_logps_forward: no response token in this (mini)batch - every label is the padding label")
        return lp["tok"], lp

    def _token_logps_dhg(self, lp, dlogp, dent=None):
        """d tok_logp [R] -> the gathered d hg [R][H] and the lm_head weight gradient (full fine-tune): logps_backward's lm-head backward
        with every row its own sequence, then the two lm-head GEMMs.  dent [R]: the gradient of the row entropies as well
        (vlr_lmhead_logps_entropy_bwd; the forward must have been asked for the entropy)"""
        ctx = lp["ctx"]
        H, V, R = self.H, self.V, lp["R"]
        acc = int(not self.grad_fresh)
        fused = bool(_hip.helper("vlr_lmhead_is_fused", R, V, H))
        lws = self._buf(("lmhead_ws", ctx["tag"], R), (int(_hip.lib().vlr_lmhead_workspace_bytes(R, V)),), torch.uint8)
        logits = None if fused else self._buf(("logits", ctx["tag"], R), (R, V), torch.float32)
        dl = self._buf(("dlogits", R), (R, V))
        if dent is not None:
            _hip.call("vlr_lmhead_logps_entropy_bwd", lp["hg"], ctx["ws"].v["lm_head"], lp["tgt"], lp["lse"], lp["entropy"],
                      dlogp.to(torch.float32).contiguous(), dent.to(torch.float32).contiguous(), dl, lws, logits, R, V, H)
        else:
            _hip.call("vlr_lmhead_logps_bwd", lp["hg"], ctx["ws"].v["lm_head"], lp["tgt"], lp["lse"], self._row_range(R + 1), R,
                      dlogp.to(torch.float32).contiguous(), 0, dl, lws, logits, R, V, H)
        dhg = torch.empty(R, H, dtype=BF16, device=self.dev)
        _hip.call("vlr_gemm_bf16", 1, dl, ctx["ws"].v["lm_head"], dhg, None, None, R, H, V, V, H, H, 0, 0, 0, 0)
        if self.lora is None:                 # under LoRA the lm_head is frozen (not a target module)
            _hip.call("vlr_gemm_bf16", 2, dl, lp["hg"], self.gv["lm_head"], None, None, V, H, R, V, H, H, 0, 0, acc, 0)
        return dhg

    def _scatter_dhg(self, lp, dhg, dhidden):
        """the gathered d hg onto its rows of the dense d hidden, then the reducer hears of the lm_head bucket"""
        _hip.call("vlr_scatter_rows", dhg, lp["rows"], dhidden, lp["R"], self.H)
        if self.reducer is not None and self.lora is None:
            self.reducer.bucket_ready("lm_head")
        return dhidden

    def token_logps_backward(self, lp, dlogp, dent=None):
        """d tok_logp [R] (and d entropy [R]) -> d hidden (dense [M,H], zero outside the response rows) and the lm_head weight gradient
        (full fine-tune)"""
        if lp["R"] == 0:
            raise ValueError("token_logps_backward: no response token in this (mini)batch")
        dhidden = torch.zeros(lp["ctx"]["M"], self.H, dtype=BF16, device=self.dev)
        return self._scatter_dhg(lp, self._token_logps_dhg(lp, dlogp, dent), dhidden)

    def ppo_forward(self, ctx, labels, label_pad=-100, entropy=False):
        """per-token log-probs and values on the R response rows (the rows whose logits predict a label != label_pad; trl reads
        values[:, :-1] under the same mask): token_logps_forward and vlr_rm_head_fwd with the value head on the same gathered rows.
        Returns (tok_logp [R] fp32, values [R] fp32, lp_ctx); lp_ctx["seq_off"] delimits the sequences.  entropy: lp_ctx["entropy"] [R]
        as in token_logps_forward (a statistic: PPO has no entropy gradient)."""
        tok, lp = self.token_logps_forward(ctx, labels, label_pad, entropy)
        R = lp["R"]
        w, b, _, _ = self.v_head_views()
        values = torch.empty(R, dtype=torch.float32, device=self.dev)
        _hip.call("vlr_rm_head_fwd", lp["hg"], self.H, self._row_range(R), w, b, values, R, self.H)
        return tok, values, lp

    def ppo_backward(self, lp, dlogp, dvalues):
        """d tok_logp [R], d values [R] -> d hidden (dense [M,H], zero outside the response rows), the lm_head weight gradient (full
        fine-tune) and the value head's gradients.  The lm-head backward is token_logps_backward's; the value head adds g_r * w onto the
        same gathered d hg before the scatter (vlr_v_head_bwd)."""
        R, H = lp["R"], self.H
        if R == 0:
            raise ValueError("ppo_backward: no response token in this (mini)batch")
        acc = int(not self.grad_fresh)
        dhidden = torch.zeros(lp["ctx"]["M"], H, dtype=BF16, device=self.dev)
        dhg = self._token_logps_dhg(lp, dlogp)
        w, _, gw, gb = self.v_head_views()
        vws = self._buf(("v_head_ws", R), (int(_hip.lib().vlr_v_head_bwd_workspace_bytes(R, H)),), torch.uint8)
        _hip.call("vlr_v_head_bwd", lp["hg"], w, dvalues.to(torch.float32).contiguous(), dhg, gw, gb, acc, vws, R, H)
        return self._scatter_dhg(lp, dhg, dhidden)

    def logits_mean(self, ctx, lo, hi):
        """mean over [lo:hi] sequences, all positions, all vocabulary entries of the logits = mean_rows(h . sum_v W_v)/V
        (the `logits/chosen|rejected` metrics of trl's get_batch_loss_metrics, never materialising [B,S,V])."""
        ws = ctx["ws"]
        # keyed on the optimizer step / load counter: vlr_adamw_step writes the weights through raw pointers, so torch's
        # tensor version counter never moves
        key = ("wsum", id(ws), self.opt_step if ws is self.policy else -1, (self._weights_version, ws.version))
        wsum = self._ws.get(key)
        if wsum is None:
            wsum = torch.empty(self.H, dtype=torch.float32, device=self.dev)
            _hip.call("vlr_colsum_f32", ws.v["lm_head"], self.V, self.H, self.H, wsum, self._colsum_ws)
            self._ws = {k: v for k, v in self._ws.items() if not (isinstance(k, tuple) and len(k) == 4 and k[0] == "wsum" and k[1] == id(ws))}
            self._ws[key] = wsum
        S = ctx["S"]
        rd = torch.empty(ctx["M"], dtype=torch.float32, device=self.dev)
        _hip.call("vlr_rowdot", ctx["hidden"], wsum, rd, ctx["M"], self.H)
        return rd[lo * S: hi * S].mean() / self.V

    def materialize_logits(self, ctx, lo=0, hi=None):
        """Full fp32 logits [hi-lo, S, V] (debug / small shapes / callers that insist on a tensor)."""
        hi = ctx["Bn"] if hi is None else hi
        S = ctx["S"]
        n = (hi - lo) * S
        out = torch.empty(n, self.V, dtype=torch.float32, device=self.dev)
        hsl = ctx["hidden"][lo * S: hi * S]
        _hip.call("vlr_gemm_bf16", 0, hsl, ctx["ws"].v["lm_head"], out, None, None, n, self.V, self.H, self.H, self.H, self.V, 0, 0, 0, 1)
        return out.view(hi - lo, S, self.V)

    # ------------------------------------------------------------------------------------------------ backward
    def logps_backward(self, lp, dlogps):
        """d logps -> d hidden (dense [M,H], zero outside the response rows) and the lm_head weight gradient."""
        ctx = lp["ctx"]
        M, H, V, R = ctx["M"], self.H, self.V, lp["R"]
        acc = int(not self.grad_fresh)
        dhidden = torch.zeros(M, H, dtype=BF16, device=self.dev)
        if R == 0:
            if not acc and self.lora is None:
                self.gv["lm_head"].zero_()
            return dhidden
        # d logits (bf16 [R][V]): the lm-head GEMM is recomputed and its epilogue writes the gradient directly (fused shapes)
        fused = bool(_hip.helper("vlr_lmhead_is_fused", R, V, H))
        lws = self._buf(("lmhead_ws", ctx["tag"], R), (int(_hip.lib().vlr_lmhead_workspace_bytes(R, V)),), torch.uint8)
        logits = None if fused else self._buf(("logits", ctx["tag"], R), (R, V), torch.float32)
        dl = self._buf(("dlogits", R), (R, V))
        _hip.call("vlr_lmhead_logps_bwd", lp["hg"], ctx["ws"].v["lm_head"], lp["tgt"], lp["lse"], lp["seq_off"], ctx["Bn"],
                  dlogps.to(torch.float32).contiguous(), int(lp["average"]), dl, lws, logits, R, V, H)
        dhg = torch.empty(R, H, dtype=BF16, device=self.dev)
        _hip.call("vlr_gemm_bf16", 1, dl, ctx["ws"].v["lm_head"], dhg, None, None, R, H, V, V, H, H, 0, 0, 0, 0)
        if self.lora is None:                 # under LoRA the lm_head is frozen (not a target module)
            _hip.call("vlr_gemm_bf16", 2, dl, lp["hg"], self.gv["lm_head"], None, None, V, H, R, V, H, H, 0, 0, acc, 0)
        _hip.call("vlr_scatter_rows", dhg, lp["rows"], dhidden, R, H)
        if self.reducer is not None and self.lora is None:
            self.reducer.bucket_ready("lm_head")
        return dhidden

    def hidden_backward(self, ctx, dhidden):
        """Backward of forward_hidden(save=True): final norm, decoder layers L-1..0, then - in a full fine-tune - merge and projector.
        Gradients land in the flat bf16 gradient buffer (overwrite when `grad_fresh`, else accumulate).  Under LoRA only the adapters
        receive gradients: nothing below the first decoder layer is trainable (embedding, projector and vision tower are not target
        modules), so the backward stops there."""
        assert ctx["acts"] is not None, "forward_hidden(save=True) required"
        full = self.lora is None
        if not full and ctx.get("lora_seed") is None:
            raise RuntimeError("backward through a pass that ran with the adapters disabled")
        ws, M = ctx["ws"], ctx["M"]
        acc = int(not self.grad_fresh)
        dxa = self._buf(("dxa", M), (M, self.H))
        dxb = self._buf(("dxb", M), (M, self.H))
        plan = ctx.get("plan")
        if plan is not None:
            # a row-compact policy pass (full fine-tune only): the dense d hidden is folded onto the kept rows - a shared row may carry
            # a label of both sequences (an identical pair) - the final norm and the layers run at Mc rows, and d x0 is expanded with
            # zeros on the dropped rows for the unchanged embedding backward
            Mc = plan["Mc"]
            dh_c = self._buf(("dedup_dhidden", M), (M, self.H))
            _hip.call("vlr_fold_rows", dhidden, plan["compact_rows"], plan["twin"], dh_c, Mc, self.H)
            self._norm_bwd(dh_c, ctx["x_last"], ws.v["norm"], ctx["rstd_f"], None, dxa, self.gv["norm"], acc, Mc)
            cur = self._layers_backward(ctx, self._layer_bwd_compact(ctx, acc, *self._bwd_workspace(ctx)), dxa, dxb)
            nxt = dxb if cur is dxa else dxa
            _hip.call("vlr_expand_rows_zero", cur, plan["dense_own"], nxt, M, self.H)
            cur = nxt
        elif ctx.get("src_plan") is not None:
            # the dense backward on the kept rows in place (full fine-tune only): every call of the dense backward at M rows, the
            # row-wise ones reading x / rstd / gate|up at dense_src[row]
            dsrc = ctx["src_plan"]["dense_src"]
            x_last = ctx["x_last"]
            _hip.call("vlr_rmsnorm_bwd_f32_src" if x_last.dtype == torch.float32 else "vlr_rmsnorm_bwd_src", dhidden, x_last, ws.v["norm"],
                      ctx["rstd_f"], None, dxa, self.gv["norm"], acc, self._norm_ws, dsrc, M, self.H)
            cur = self._layers_backward(ctx, self._layer_bwd_src(ctx, acc, *self._bwd_workspace(ctx)), dxa, dxb)
        else:
            self._norm_bwd(dhidden, ctx["x_last"], ws.v["norm"], ctx["rstd_f"], None, dxa, self.gv["norm"] if full else None, acc if full else 0, M)
            cur = self._layers_backward(ctx, self._layer_bwd(ctx, acc, *self._bwd_workspace(ctx)), dxa, dxb)
        if full:
            self._embed_backward(ctx, cur, acc)
        self.grad_fresh = False
        if self.reducer is not None:
            self.reducer.bucket_ready("tail" if full else "lora")

    def _bwd_workspace(self, ctx):
        """scratch of one decoder layer's backward, shared by every layer: (buffers by name, the library's vlr_layer_bwd_ws over them)"""
        Bn, S, M, H = ctx["Bn"], ctx["S"], ctx["M"], self.H
        wsb = dict(dact=self._buf(("dact", M), (M, self.I)), dxn=self._buf(("dxn", M), (M, H)), dattn=self._buf(("dattn", M), (M, self.Nq)),
                   dqkv=self._buf(("dqkv", M), (M, self.Nqkv)), dx_mid=self._buf(("dx_mid", M), (M, H)),
                   delta=self._buf(("delta", Bn, S), (Bn, self.nh, _align(S, 64)), torch.float32), norm_ws=self._norm_ws)
        return wsb, _hip.LayerBwdWs(*(wsb[n].data_ptr() for n, _ in _hip.LayerBwdWs._fields_))

    def _layers_backward(self, ctx, layer_bwd, cur, nxt):
        """the decoder layers in reverse: layer_bwd(l, a, x_in, cur, nxt) turns d x_out (`cur`) into d x_in (`nxt`) and writes layer l's
        parameter gradients.  Under gradient checkpointing each layer's forward is re-run first, as the pass itself ran it (same adapters,
        same dropout seeds).  -> the gradient of the decoder's input"""
        ws, Bn, S = ctx["ws"], ctx["Bn"], ctx["S"]
        plan = ctx.get("plan")           # a row-compact policy pass: the layer inputs are its kept rows, the recompute is the compact forward
        if plan is not None and ctx["ckpt"]:
            qkv_d, attn_d = (self._buf((ctx["tag"], k, Bn, S), (ctx["M"], n)) for k, n in (("dedup_qkv", self.Nqkv), ("dedup_attn", self.Nq)))
        for l in range(self.L - 1, -1, -1):
            a = ctx["acts"][l]
            kept = plan is not None or ctx.get("src_plan") is not None      # the layer inputs are the pass's kept rows
            x_in = ctx["acts"][l - 1]["x_out"] if l > 0 else (ctx["x0_c"] if kept else ctx["x0"])
            if ctx["ckpt"] and plan is not None:
                self._layer_fwd_compact_call(ws, l, a, x_in, ctx["embed"], plan, qkv_d, attn_d, Bn, S, True)
            elif ctx["ckpt"]:
                self._layer_fwd_call(ws, l, a, x_in, ctx["embed"], Bn, S, True, ctx["use_lora"], ctx["lora_seed"])
            layer_bwd(l, a, x_in, cur, nxt)
            cur, nxt = nxt, cur
            if self.lora is None and self.reducer is not None:       # (LoRA: one bucket when the backward is done)
                self.reducer.bucket_ready(f"layer{l}")
        return cur

    def _layer_bwd_compact(self, ctx, acc, wsb, lws):
        """the per-layer backward of a row-compact policy pass (ctx["plan"]), for _layers_backward: vlr_decoder_layer_bwd_compact over the
        backward's own scratch (its first Mc rows) and four dense operands of the attention backward"""
        ws, Bn, S, M, plan = ctx["ws"], ctx["Bn"], ctx["S"], ctx["M"], ctx["plan"]
        tag = ctx["tag"]
        dense = dict(qkv=self._buf((tag, "dedup_qkv", Bn, S), (M, self.Nqkv)), attn=self._buf((tag, "dedup_attn", Bn, S), (M, self.Nq)),
                     dattn=self._buf((tag, "dedup_dattn", Bn, S), (M, self.Nq)), dqkv=self._buf((tag, "dedup_dqkv", Bn, S), (M, self.Nqkv)))
        ds = _hip.DenseScratch(*(dense[n].data_ptr() for n, _ in _hip.DenseScratch._fields_))

        def compact(l, a, x_in, cur, nxt):
            _hip.call("vlr_decoder_layer_bwd_compact", self.llama_cfg, self.layer_weights(ws, l, tag), self.layer_grads(l), acc, a["struct"],
                      lws, plan["struct"], ds, x_in, cur, nxt, ctx["mask"], Bn, S)
            if f"l{l}.bqkv" in self.gv:          # (the folded d qkv of the kept rows: a shared row's entry is already the sum of its two copies)
                _hip.call("vlr_colsum", wsb["dqkv"], plan["Mc"], self.Nqkv, self.Nqkv, self.gv[f"l{l}.bqkv"], acc, self._colsum_ws)
        return compact

    def _layer_bwd_src(self, ctx, acc, wsb, lws):
        """the per-layer backward after _forward_layers_compact_keep (ctx["src_plan"]), for _layers_backward: vlr_decoder_layer_bwd_src
        over the dense backward's scratch and one [M][2I] buffer for d gate | d up, shared by all layers"""
        ws, Bn, S, M, plan = ctx["ws"], ctx["Bn"], ctx["S"], ctx["M"], ctx["src_plan"]
        dgu = self._buf(("dgu", M), (M, 2 * self.I))

        def src(l, a, x_in, cur, nxt):
            _hip.call("vlr_decoder_layer_bwd_src", self.llama_cfg, self.layer_weights(ws, l, ctx["tag"]), self.layer_grads(l), acc, a["struct"],
                      lws, dgu, plan["dense_src"], x_in, cur, nxt, ctx["pos"], ctx["mask"], Bn, S)
            if f"l{l}.bqkv" in self.gv:          # bias of the fused q|k|v projection: column sum of this layer's d qkv (post rope-transpose)
                _hip.call("vlr_colsum", wsb["dqkv"], M, self.Nqkv, self.Nqkv, self.gv[f"l{l}.bqkv"], acc, self._colsum_ws)
        return src

    def _layer_bwd(self, ctx, acc, wsb, lws):
        """the per-layer backward of this engine's current mode, for _layers_backward"""
        ws, Bn, S, M = ctx["ws"], ctx["Bn"], ctx["S"], ctx["M"]
        if self.lora is None:
            def full(l, a, x_in, cur, nxt):
                _hip.call("vlr_decoder_layer_bwd", self.llama_cfg, self.layer_weights(ws, l, ctx["tag"]), self.layer_grads(l), acc,
                          a["struct"], lws, x_in, cur, nxt, ctx["pos"], ctx["mask"], Bn, S)
                if f"l{l}.bqkv" in self.gv:          # bias of the fused q|k|v projection: column sum of this layer's d qkv (post rope-transpose)
                    _hip.call("vlr_colsum", wsb["dqkv"], M, self.Nqkv, self.Nqkv, self.gv[f"l{l}.bqkv"], acc, self._colsum_ws)
            return full
        # data gradients through the frozen decoder + adapter gradients
        ws_v = self._buf(("lora_v", M), (M, 3 * self.lora["r"]))
        drop = self.lora["dropout"] > 0 and self.training
        scratch = self._buf(("lora_scratch", M), (M, max(self.H, self.I))) if drop else None     # fallback path of the fused dropout-accumulate

        def lora(l, a, x_in, cur, nxt):
            lw, lg = self._lora_structs(l, train=True, M=M, acts=a)
            _hip.call("vlr_decoder_layer_bwd_lora", self.llama_cfg, self.layer_weights(ws, l, ctx["tag"]), lw, lg, acc, a["struct"],
                      a.get("shared", a)["u"], lws, ws_v, scratch, ctx["lora_seed"] + 8 * l, x_in, cur, nxt, ctx["pos"], ctx["mask"], Bn, S)
        return lora

    def _embed_backward(self, ctx, cur, acc):
        """gradient of the merged embeddings `cur` [M,H] -> embed_tokens rows, projector (and image_newline) gradients"""
        ws = ctx["ws"]
        Bn, S, H = ctx["Bn"], ctx["S"], self.H
        # ---- merge + projector
        n_rows, dup = ctx["n_rows"], ctx["image_dup"]
        if not acc:
            self.gv["embed"].zero_()          # rows of tokens that do not occur keep a zero gradient
        if ctx["pack"] is None:
            dfeats = self._buf(("dfeats", n_rows), (n_rows, H))
            _hip.call("vlr_merge_bwd", cur, ctx["src"], ctx["inv"], ctx["ids"], dfeats, self.gv["embed"], Bn, ctx["T"], S, H, n_rows, dup)
        else:
            # LLaVA-Next: gradient of the packed rows, then un-pack: every projector row feeds at most one packed row (tiles the
            # un-padding dropped get zero), the image_newline row feeds one packed row per grid line -> fixed-order column sum
            pk = ctx["pack"]
            F = pk["F"]
            dpacked = self._buf(("dpacked", F), (F, H))
            _hip.call("vlr_merge_bwd", cur, ctx["src"], ctx["inv"], ctx["ids"], dpacked, self.gv["embed"], Bn, ctx["T"], S, H, F, dup)
            dext = self._buf(("dfeats_ext", n_rows), (n_rows + 1, H))
            dext.zero_()
            _hip.call("vlr_scatter_rows", dpacked, pk["idx"], dext, F, H)
            n_nl = int(pk["nl"].shape[0])
            dnl = self._buf(("dnewline", n_nl), (n_nl, H))
            _hip.call("vlr_gather_rows", dpacked, pk["nl"], dnl, n_nl, H)
            _hip.call("vlr_colsum", dnl, n_nl, H, H, self.gv["image_newline"], acc, self._colsum_ws)
            dfeats = dext[:n_rows]
        D = self.D
        _hip.call("vlr_colsum", dfeats, n_rows, H, H, self.gv["proj.b2"], acc, self._colsum_ws)
        _hip.call("vlr_gemm_bf16", 2, dfeats, ctx["proj_h"], self.gv["proj.w2"], None, None, H, H, n_rows, H, H, H, 0, 0, acc, 0)
        dh = self._buf(("proj_dh", n_rows), (n_rows, H))
        _hip.call("vlr_gemm_bf16", 1, dfeats, ws.v["proj.w2"], dh, None, None, n_rows, H, H, H, H, H, 0, 0, 0, 0)
        dz = self._buf(("proj_dz", n_rows), (n_rows, H))
        _hip.call("vlr_gelu_bwd", ctx["proj_z"], dh, dz, dz.numel())
        _hip.call("vlr_colsum", dz, n_rows, H, H, self.gv["proj.b1"], acc, self._colsum_ws)
        _hip.call("vlr_gemm_bf16", 2, dz, ctx["vit_feat"], self.gv["proj.w1"], None, None, H, D, n_rows, H, D, D, 0, 0, acc, 0)
        if ctx.get("vit_keep"):
            self._vision_backward(ctx, ctx["vit_keep"], dz, acc)

    def make_reducer(self, group=None):
        """DDP gradient reducer over the trainable flat gradient buffer (full fine-tuning: one bucket per decoder layer in
        backward order; LoRA: the adapters are small, one bucket when the backward is done)."""
        from .parallel import GradReducer
        if self.lora is not None:
            self.reducer = GradReducer(self.lora_grads, {"lora": (0, self.lora_layout.numel)}, group=group)
        else:
            self.reducer = GradReducer(self.grads, self.layout.bucket_after, group=group)
        return self.reducer

    # ------------------------------------------------------------------------------------------------ optimizer
    def init_optimizer(self):
        """fp32 master copy + Adam moments for the flat parameter buffer (28 B of HBM traffic per parameter and step).
        The reference leaves the precision policy to DeepSpeed/DDP; fp32 master + fp32 moments is the documented choice."""
        self.master = (self.lora_flat if self.lora is not None else self.policy.flat).float()
        self.m = torch.zeros_like(self.master)
        self.v = torch.zeros_like(self.master)
        self.opt_step = 0

    def optimizer_state(self):
        """fp32 master / m / v + step counter (what torch.optim.AdamW.state_dict() carries), for checkpoints."""
        if self.master is None:
            return None
        self.wait_optimizer()
        return dict(master=self.master, m=self.m, v=self.v, opt_step=self.opt_step)

    def load_optimizer_state(self, master, m, v, opt_step):
        if self.master is None:
            self.init_optimizer()
        for dst, src in ((self.master, master), (self.m, m), (self.v, v)):
            if dst.numel() != src.numel():
                raise ValueError(f"optimizer state has {src.numel()} elements, the trainable buffer {dst.numel()}")
            dst.copy_(src.to(self.dev))
        self.opt_step = int(opt_step)
        # the bf16 working copy is the rounding of the master weights
        (self.lora_flat if self.lora is not None else self.policy.flat).copy_(self.master)
        self._vit_cache_policy = None
        self._weights_version += 1

    def zero_grad(self):
        self.grad_fresh = True

    def wait_optimizer(self):
        """order the current stream behind the last optimizer step.  The step runs on the caller's stream (on a stream of its own it
        measured no gain: 650.7 / 652.6 ms without, 648.5 / 653.1 ms with), so there is nothing to wait for; kept for callers."""

    def grad_norm(self) -> float:
        """total gradient norm of the last optimizer step (host value; synchronises)"""
        return float(self.norm_out[0])

    def optimizer_step(self, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_grad_norm=1.0, grad_scale=1.0):
        """clip + AdamW on the caller's stream, behind the gradient exchange."""
        if self.master is None:
            self.init_optimizer()
        if self.reducer is not None:
            self.reducer.wait()
        return self._optimizer_step(lr, beta1, beta2, eps, weight_decay, max_grad_norm, grad_scale)

    def _optimizer_step(self, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_grad_norm=1.0, grad_scale=1.0):
        """clip_grad_norm_(max_grad_norm) + AdamW on the flat buffers; no host synchronisation (the clip coefficient
        stays on the device).  grad_scale multiplies the raw gradients first (1/world_size after a sum all-reduce,
        1/gradient_accumulation_steps ...).  Returns the device tensor [norm, coef, sum g^2]."""
        if self.master is None:
            self.init_optimizer()
        if self.reducer is not None:
            self.reducer.wait()
        if self.lora is not None:
            # HF's decay grouping puts every lora_A / lora_B weight in the decay group.
            n = self.lora_layout.numel
            _hip.call("vlr_grad_sqnorm", self.lora_grads, n, float(max_grad_norm if max_grad_norm else 0.0),
                      float(grad_scale), 0.0, self._sq_ws, self.norm_out)
            self.opt_step += 1
            nd = self.lora_layout.n_decay
            for lo, hi, wd in ((0, nd, weight_decay), (nd, n, 0.0)):      # (the no-decay tail is the reward head's bias, when there is one)
                if hi <= lo:
                    continue
                _hip.call("vlr_adamw_step", self.master[lo:hi], self.m[lo:hi], self.v[lo:hi], self.lora_grads[lo:hi], self.lora_flat[lo:hi],
                          hi - lo, float(lr), float(beta1), float(beta2), float(eps), float(wd), self.opt_step, self.norm_out)
            self.grad_fresh = True
            return self.norm_out
        n = self.layout.n_opt
        _hip.call("vlr_grad_sqnorm", self.grads, n, float(max_grad_norm if max_grad_norm else 0.0), float(grad_scale), 0.0,
                  self._sq_ws, self.norm_out)
        self.opt_step += 1
        nd = self.layout.n_decay
        for lo, hi, wd in ((0, nd, weight_decay), (nd, n, 0.0)):
            if hi <= lo:              # (InternLM-XComposer2: no bias / nn.LayerNorm parameter is trainable - the no-decay region is empty)
                continue
            _hip.call("vlr_adamw_step", self.master[lo:hi], self.m[lo:hi], self.v[lo:hi], self.grads[lo:hi],
                      self.policy.flat[lo:hi], hi - lo, float(lr), float(beta1), float(beta2), float(eps), float(wd),
                      self.opt_step, self.norm_out)
        self._vit_cache_policy = None      # (the trainable tower moved)
        self.grad_fresh = True
        return self.norm_out
