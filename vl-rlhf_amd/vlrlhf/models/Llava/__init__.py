"""LLaVA-1.5 wrapper for the MI355X DPO path - mirror of /root/reference/src/vlrlhf/models/Llava/__init__.py
(LlavaRLOutputWithPast :22-32, LlavaForRL :35-298, LlavaProcessor :315-432, LlavaDPODataCollatorWithPadding :435-443,
LlavaDPOTrainer :474, core_mapper :486-499).  `LlavaForRL.forward` keeps the reference call signature and output
fields; underneath it runs vlrlhf.engine (HIP kernels) and returns a LAZY logits handle so the [2B,S,V] fp32 tensor is
never written to HBM unless a caller asks for it."""
import contextlib
import json
import os
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, List, Literal, Optional, Tuple, Union

import torch
import torch.nn as nn

from ... import _hip, gptq
from ...base.collator import VLDPODataCollatorWithPadding, VLPPODataCollator, VLRMDataCollatorWithPadding, VLSFTDataCollatorWithPadding
from ...base.model import VLModelWithValueHead, VLRewardModel
from ...base.processor import VLChatTemplate, VLProcessor
from ...base.trainer import VLDPOTrainer, VLGRPOTrainer, VLKTOTrainer, VLPPOTrainer, VLRMTrainer, VLSFTTrainer
from ...engine import BF16, LlavaHipEngine, WeightSet
from ...utils.common import flatten_list
from ..utils import GRPOCore, KTOCore, ModelCoreMapper, PPOCore


@dataclass
class LlavaRLOutputWithPast:
    loss: Optional[torch.Tensor] = None
    logits: Any = None
    past_key_values: Optional[List[torch.Tensor]] = None
    hidden_states: Optional[Tuple[torch.Tensor]] = None
    attentions: Optional[Tuple[torch.Tensor]] = None
    image_hidden_states: Optional[Tuple[torch.Tensor]] = None
    labels: Optional[torch.Tensor] = None
    image_position_map: Optional[torch.Tensor] = None
    # the reference computes the causal-LM cross-entropy in every forward(labels=...) and DPO throws it away; here `loss` is computed
    # on FIRST ACCESS (one lm-head pass over the label rows), so a caller that never reads it - the DPO path - launches nothing for it
    loss_fn: Optional[Callable[[], torch.Tensor]] = field(default=None, repr=False, compare=False)

    def __getattribute__(self, name):
        if name == "loss":
            d = object.__getattribute__(self, "__dict__")
            if d.get("loss") is None and d.get("loss_fn") is not None:
                d["loss"], d["loss_fn"] = d["loss_fn"](), None
            return d.get("loss")
        return object.__getattribute__(self, name)

    def __getitem__(self, k):
        return getattr(self, k) if isinstance(k, str) else (self.loss, self.logits)[k]


# ----------------------------------------------------------------------------------------------------------
class _HiddenFn(torch.autograd.Function):
    """embed -> ViT -> projector -> merge -> 32 decoder layers -> final norm, as ONE autograd node.  Parameter
    gradients are written by the HIP backward straight into the engine's flat gradient buffer (the .grad of every
    nn.Parameter is a view of it), so this node returns no tensor gradients."""

    @staticmethod
    def forward(ctx, anchor, model, input_ids, attention_mask, labels, pixel_values, dup, image_sizes=None):
        c = model.engine.forward_hidden(model.weights, input_ids, attention_mask, labels, pixel_values, image_dup=dup,
                                        save=True, tag="policy", image_sizes=image_sizes,
                                        prefix_dedup_rows=bool(getattr(model, "_policy_pass", False)))
        ctx.c, ctx.engine = c, model.engine
        model._last_ctx = c
        return c["hidden"]

    @staticmethod
    def backward(ctx, dhidden):
        ctx.engine.hidden_backward(ctx.c, dhidden.contiguous())
        ctx.c = None
        return (None,) * 8


class _LogpsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hidden, engine, c, labels, shared, average, label_pad):
        logps, lp = engine.logps_forward(c, labels, shared, average, label_pad)
        ctx.lp, ctx.engine = lp, engine
        return logps

    @staticmethod
    def backward(ctx, dlogps):
        dh = ctx.engine.logps_backward(ctx.lp, dlogps.contiguous())
        ctx.lp = None
        return (dh,) + (None,) * 6


class _CeFn(torch.autograd.Function):
    """batch-mean cross-entropy over the label rows (engine.ce_forward / ce_backward) as one autograd node returning the scalar"""

    @staticmethod
    def forward(ctx, hidden, engine, c, labels, shift_mask, label_pad):
        out3, lp = engine.ce_forward(c, labels, shift_mask, label_pad)
        ctx.lp, ctx.engine = lp, engine
        return out3[0].clone()

    @staticmethod
    def backward(ctx, dloss):
        dh = ctx.engine.ce_backward(ctx.lp, dloss)
        ctx.lp = None
        return (dh,) + (None,) * 5


class LazyLogits:
    """Stand-in for the [B,S,V] logits of the reference (`output.logits`): supports what the DPO path does with them -
    `get_batch_logps` (fused lm-head + log-softmax pick on the response rows), batch slicing, `.detach()`, `.mean()`
    (trl's logits/* metrics) - and `materialize()` for callers that need the tensor."""

    def __init__(self, engine, c, hidden, lo=0, hi=None):
        self.engine, self.c, self.hidden = engine, c, hidden
        self.lo, self.hi = lo, (c["Bn"] if hi is None else hi)

    @property
    def shape(self):
        return torch.Size((self.hi - self.lo, self.c["S"], self.engine.V))

    @property
    def dtype(self):
        return torch.float32

    @property
    def device(self):
        return self.engine.dev

    is_cuda = True

    def __getitem__(self, idx):
        if isinstance(idx, slice):
            lo, hi, st = idx.indices(self.hi - self.lo)
            assert st == 1
            return LazyLogits(self.engine, self.c, self.hidden, self.lo + lo, self.lo + hi)
        return self.materialize()[idx]

    def detach(self):
        return LazyLogits(self.engine, self.c, self.hidden.detach(), self.lo, self.hi)

    def float(self):
        return self

    def to(self, *a, **k):
        return self

    def mean(self):
        return self.engine.logits_mean(self.c, self.lo, self.hi)

    def materialize(self):
        return self.engine.materialize_logits(self.c, self.lo, self.hi)

    def batch_logps(self, labels, shared, average, label_pad):
        assert self.lo == 0 and self.hi == self.c["Bn"], "get_batch_logps expects the whole concatenated batch"
        if self.hidden.requires_grad:
            return _LogpsFn.apply(self.hidden, self.engine, self.c, labels, shared, bool(average), int(label_pad))
        logps, _ = self.engine.logps_forward(self.c, labels, shared, bool(average), int(label_pad))
        return logps

    def cross_entropy(self, labels, shift_mask=None, label_pad=-100):
        """nn.CrossEntropyLoss()(shift_logits[sel], shift_labels[sel]) of the reference wrappers (scalar; differentiable when the forward
        was): sel = shifted positions with label != label_pad and, when given, shift_mask [B, S-1] != 0."""
        assert self.lo == 0 and self.hi == self.c["Bn"], "the loss is a mean over the whole batch"
        if self.hidden.requires_grad:
            return _CeFn.apply(self.hidden, self.engine, self.c, labels, shift_mask, int(label_pad))
        out3, _ = self.engine.ce_forward(self.c, labels, shift_mask, int(label_pad))
        return out3[0].clone()


class _Config(dict):
    """attribute + dict access; the handful of HF config fields the reference reads."""
    __getattr__ = dict.get

    def __setattr__(self, k, v):
        self[k] = v


def _cfg_from_hf(hf: dict) -> dict:
    t, v = hf.get("text_config", {}), hf.get("vision_config", {})
    hidden = t.get("hidden_size", 4096)
    extra = {}
    if t.get("num_key_value_heads") and t["num_key_value_heads"] != t.get("num_attention_heads", 32):
        extra["kv_heads"] = t["num_key_value_heads"]
    if hf.get("image_grid_pinpoints"):
        extra["image_grid_pinpoints"] = [list(p) for p in hf["image_grid_pinpoints"]]
    return dict(
        **extra,
        vit_hidden=v.get("hidden_size", 1024), vit_mlp=v.get("intermediate_size", 4096),
        vit_layers=v.get("num_hidden_layers", 24), vit_heads=v.get("num_attention_heads", 16),
        image_size=v.get("image_size", 336), patch_size=v.get("patch_size", 14), vit_ln_eps=v.get("layer_norm_eps", 1e-5),
        hidden=hidden, inter=t.get("intermediate_size", 11008), layers=t.get("num_hidden_layers", 32),
        heads=t.get("num_attention_heads", 32), vocab=t.get("vocab_size", hf.get("vocab_size", 32064)),
        rms_eps=t.get("rms_norm_eps", 1e-5), rope_theta=t.get("rope_theta", 10000.0),
        image_token=hf.get("image_token_index", 32000), model_pad_token_id=hf.get("pad_token_id", 32001),
        ignore_index=hf.get("ignore_index", -100))


def _hf_from_cfg(c: dict) -> dict:
    """config.json (transformers==4.41.0 LlavaConfig / LlavaNextConfig layout) for a model that was not loaded from a checkpoint."""
    nxt = bool(c.get("image_grid_pinpoints"))
    return dict(
        **({"image_grid_pinpoints": c["image_grid_pinpoints"]} if nxt else {}),
        architectures=["LlavaNextForConditionalGeneration" if nxt else "LlavaForConditionalGeneration"],
        model_type="llava_next" if nxt else "llava", image_token_index=c["image_token"],
        pad_token_id=c.get("model_pad_token_id", c["image_token"] + 1), ignore_index=c.get("ignore_index", -100),
        projector_hidden_act="gelu", vision_feature_layer=-2, vision_feature_select_strategy="default",
        vocab_size=c["vocab"], torch_dtype="bfloat16",
        text_config=dict(model_type="mistral" if nxt and c.get("kv_heads") else "llama", hidden_size=c["hidden"], intermediate_size=c["inter"], num_hidden_layers=c["layers"],
                         num_attention_heads=c["heads"], num_key_value_heads=c.get("kv_heads", c["heads"]), vocab_size=c["vocab"],
                         rms_norm_eps=c.get("rms_eps", 1e-5), rope_theta=c.get("rope_theta", 10000.0)),
        vision_config=dict(model_type="clip_vision_model", hidden_size=c["vit_hidden"], intermediate_size=c["vit_mlp"],
                           num_hidden_layers=c["vit_layers"], num_attention_heads=c["vit_heads"], image_size=c["image_size"],
                           patch_size=c["patch_size"], layer_norm_eps=c.get("vit_ln_eps", 1e-5)))


def sampling_filter(logits, temperature=1.0, top_k=50, top_p=1.0):
    """transformers' logits warpers in their order (TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper): the filtered-out entries
    become -inf; at least one token always survives"""
    logits = logits / max(float(temperature), 1e-6)
    if top_k and top_k > 0:
        kth = torch.topk(logits, min(int(top_k), logits.shape[-1]), dim=-1).values[:, -1:]
        logits = logits.masked_fill(logits < kth, float("-inf"))
    if top_p < 1.0:
        srt, idx = torch.sort(logits, dim=-1, descending=False)
        drop = srt.softmax(-1).cumsum(-1) <= (1.0 - float(top_p))
        drop[:, -1] = False
        logits = logits.masked_fill(drop.scatter(1, idx, drop), float("-inf"))
    return logits


def stop_sequences(stop_words_ids, device):
    """generation_config.stop_words_ids (a list of token-id lists; Qwen-VL's generation config, InternLM-XComposer2's end-of-turn id) ->
    one 1-D id tensor per non-empty sequence on `device`, uploaded once per generate call"""
    if not stop_words_ids:
        return []
    if isinstance(stop_words_ids[0], int):
        raise ValueError(f"stop_words_ids must be a list of token-id lists, got {stop_words_ids}")
    return [torch.tensor([int(x) for x in s], dtype=torch.long, device=device) for s in stop_words_ids if len(s)]


def stop_hit(generated, stops):
    """bool [B]: rows whose GENERATED tokens ([B, n], the prompt never counts) end with one of `stops`.  Tensor compares of the last k
    columns on the device; nothing is read back."""
    hit = torch.zeros(generated.shape[0], dtype=torch.bool, device=generated.device)
    for s in stops:
        k = s.numel()
        if generated.shape[1] >= k:
            hit = hit | (generated[:, -k:] == s).all(1)
    return hit


class DeviceSampler:
    """generate's per-token selection on the device (sampler="device"): ONE vlr_sample_tokens launch per new token (include/vlr.h
    "sampling") does the logits-processor chain, the counter-based draw, the log-prob and the eos bookkeeping on the fp32 logits the
    lm-head left in HBM.  Both routes of generate (KV cache and re-forward) select through select(); every buffer is allocated here,
    once per call:
      full [rows][limit] int64   prompt + generated ids; the kernel writes column T0 + step itself (no cat),
      logp [limit - T0][rows]    the drawn tokens' log-probs, step-major so that one step's slice is contiguous (0 at pad positions),
      unfinished [rows] uint8, finish [rows] int32 (the step at which a row finished, -1 while it runs), nxt [rows] int32 (what
      decode_step consumes).
    The penalty reads the prompt as `prompt` [rows / div][T0] through prompt_div = div (the num_return_sequences fan-out keeps one copy).
    The RNG counter is (column / 4, row, step, call) under the key `seed`: a row's draw depends on its index in the expanded batch, the
    step, the model's call counter and the seed - not on the batch around it.  Stop sequences are matched after the launch by stop_hit,
    as on the torch path.  The host looks at `unfinished` every `sync_every` tokens only; result() trims to the column at which a
    per-token check would have stopped, so the output is the same for every sync_every >= 1."""

    def __init__(self, prompt, div, limit, do_sample, temperature, top_k, top_p, penalty, eos, pad, seed, call, stops=(), sync_every=8):
        dev = prompt.device
        P, T0 = prompt.shape
        self.rows, self.T0, self.max_new, self.div = P * div, T0, limit - T0, div
        self.prompt = prompt.contiguous()
        self.full = torch.full((self.rows, limit), pad, dtype=torch.long, device=dev)
        self.full[:, :T0] = prompt.repeat_interleave(div, 0) if div > 1 else prompt
        self.gen = self.full[:, T0:]
        self.logp = torch.zeros(max(self.max_new, 1), self.rows, dtype=torch.float32, device=dev)
        self.unfinished = torch.ones(self.rows, dtype=torch.uint8, device=dev)
        self.finish = torch.full((self.rows,), -1, dtype=torch.int32, device=dev)
        self.nxt = torch.empty(self.rows, dtype=torch.int32, device=dev)
        eos = sorted(int(e) for e in eos)
        if len(eos) > 8:
            raise ValueError(f'sampler="device" takes at most 8 eos ids, got {len(eos)}')
        self.eos = torch.tensor(eos, dtype=torch.int32, device=dev) if eos else None
        self.n_eos = len(eos)
        self.warp = (int(bool(do_sample)), float(temperature), int(top_k or 0), float(top_p), float(penalty))
        self.pad, self.seed, self.call = int(pad), int(seed) & 0xFFFFFFFFFFFFFFFF, int(call) & 0xFFFFFFFF
        self.stops, self.keep = stops, max((s.numel() for s in stops), default=0)
        self.sync_every = max(1, int(sync_every))
        self.n = 0

    def select(self, logits):
        """logits fp32 [rows][V] (any row stride) -> the next tokens [rows] int32; column T0 + n of `full`, logp[n], unfinished and finish
        are updated on the device"""
        n = self.n
        _hip.call("vlr_sample_tokens", logits, self.rows, logits.shape[1], logits.stride(0), *self.warp, self.prompt, self.T0, self.T0,
                  self.div, self.gen, self.full.shape[1], n, self.eos, self.n_eos, self.pad, self.seed, self.call, n, None,
                  self.unfinished, self.nxt, self.gen, self.full.shape[1], self.logp[n], self.finish, None)
        self.n = n + 1
        if self.stops:      # the stop tokens stay in the row; from the next position on it receives the pad id
            hit = stop_hit(self.gen[:, max(0, self.n - self.keep):self.n], self.stops) & (self.unfinished != 0)
            self.finish.masked_fill_(hit, n)
            self.unfinished.masked_fill_(hit, 0)
        return self.nxt

    def done(self):
        """the loop's end: the token budget, or (looked at every sync_every tokens: one host round trip) no row left unfinished"""
        if self.n >= self.max_new:
            return True
        return self.n % self.sync_every == 0 and not bool(self.unfinished.any())

    def result(self, output_logprobs=False):
        """prompt + continuation ids [rows][T0 + cols] (and the log-probs [rows][cols]): cols = the column after which a per-token
        check would have stopped - the last finish step + 1 when every row has finished, else all n"""
        cols = self.n
        if self.n and not bool(self.unfinished.any()):
            cols = int(self.finish.max()) + 1
        ids = self.full[:, :self.T0 + cols].contiguous()
        return (ids, self.logp[:cols].t().contiguous()) if output_logprobs else ids


class LlavaForRL(nn.Module):
    engine_cls = LlavaHipEngine
    image_count_key = "image_token"      # engine cfg key of the id that marks one image in input_ids (the online-RL trainers cut image inputs by it)

    def __init__(self, cfg: dict, engine: Optional[LlavaHipEngine] = None, weights: Optional[WeightSet] = None,
                 trainable: bool = True):
        super().__init__()
        self.engine = engine if engine is not None else self.engine_cls(cfg)
        self.weights = weights if weights is not None else self.engine.policy
        self.config = _Config(cfg)
        self.config.setdefault("is_encoder_decoder", False)
        self.config.setdefault("image_token_index", cfg.get("image_token", -1))
        self.config.setdefault("ignore_index", -100)
        self.config.setdefault("use_cache", False)
        self.pad_token_id = cfg.get("model_pad_token_id", cfg.get("image_token", -1) + 1)
        self._trainable = trainable and self.weights is self.engine.policy
        self._params = nn.ParameterDict()
        self._hf_names = {}
        if self._trainable:
            sd = self.weights.state_dict()
            for i, (hf, v) in enumerate(sd.items()):
                p = nn.Parameter(v, requires_grad=True)
                self._params[f"p{i}"] = p
                self._hf_names[f"_params.p{i}"] = hf
            gsd = WeightSet(self.engine.layout, self.engine.dev, self.engine.grads).state_dict()
            for i, hf in enumerate(sd.keys()):
                self._params[f"p{i}"].grad = gsd[hf]
        self._anchor = nn.Parameter(torch.zeros(1, device=self.engine.dev), requires_grad=True)
        self._last_ctx = None
        self._vision_frozen = not self.engine.train_vision      # cfg["train_vision_tower"]: the tower's evaluated tensors are parameters

    # ---- construction ---------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, cfg: dict, sd: Dict[str, torch.Tensor], **kw):
        m = cls(cfg, **kw)
        m.engine.load_state_dict(sd)
        return m

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *args, torch_dtype=None, use_flash_attention_2=None, train_vision_tower=False,
                        **kwargs):
        """reads a transformers==4.41.0 LLaVA checkpoint directory (config.json + *.safetensors).  train_vision_tower
        (--freeze_vision_tower False): the CLIP tower's evaluated tensors join the trainable parameters."""
        from safetensors.torch import load_file
        path = pretrained_model_name_or_path
        with open(os.path.join(path, "config.json")) as f:
            hf = json.load(f)
        cfg = _cfg_from_hf(hf)
        # a GPTQ checkpoint (quantization_config) loads PACKED: the decoder projections stay int4 on the device (vlrlhf/gptq.py);
        # embedding, lm-head, norms, biases, vision tower and projector are bf16 as always
        quant = gptq.parse_quantization_config(hf)
        if quant:
            cfg["gptq"] = quant
        if train_vision_tower:
            cfg["train_vision_tower"] = True
        m = cls(cfg)
        m.hf_config = hf
        sd = {}
        idx = os.path.join(path, "model.safetensors.index.json")
        files = sorted(set(json.load(open(idx))["weight_map"].values())) if os.path.exists(idx) else \
            [f for f in os.listdir(path) if f.endswith(".safetensors")]
        for fn in files:
            sd.update(load_file(os.path.join(path, fn)))
        m.engine.load_state_dict(sd)
        return m

    def save_pretrained(self, output_dir, max_shard_bytes: int = 5 << 30, state_dict=None):
        """Writes a directory `from_pretrained` (and transformers) can load: config.json + sharded safetensors of the WHOLE
        model - language model, projector and the frozen vision tower's original tensors (reference: HF Trainer._save ->
        model.save_pretrained).  `state_dict`: alternative LLM/projector tensors (e.g. merge_and_unload())."""
        from safetensors.torch import save_file
        if self.is_packed:
            raise NotImplementedError("save_pretrained: a model over GPTQ int4 base weights is not written back as a whole (peft saves the "
                                      "adapter of a GPTQ model, never the base); use save_adapter")
        os.makedirs(output_dir, exist_ok=True)
        hf = dict(getattr(self, "hf_config", None) or _hf_from_cfg(self.engine.cfg))
        hf.setdefault("architectures", ["LlavaForConditionalGeneration"])
        with open(os.path.join(output_dir, "config.json"), "w") as f:
            json.dump(hf, f, indent=1)
        sd = dict(state_dict if state_dict is not None else self.state_dict())
        for k, v in self.engine.vision_sd.items():      # the frozen copy; a trained tower's tensors are in the state dict already
            sd.setdefault(k, v)
        shards, cur, size = [], {}, 0
        for k, v in sd.items():
            nb = v.numel() * v.element_size()
            if cur and size + nb > max_shard_bytes:
                shards.append(cur)
                cur, size = {}, 0
            cur[k] = v
            size += nb
        shards.append(cur)
        if len(shards) == 1:
            save_file({k: v.detach().contiguous().cpu() for k, v in shards[0].items()}, os.path.join(output_dir, "model.safetensors"))
            return
        wmap = {}
        for i, sh in enumerate(shards):
            fn = f"model-{i + 1:05d}-of-{len(shards):05d}.safetensors"
            save_file({k: v.detach().contiguous().cpu() for k, v in sh.items()}, os.path.join(output_dir, fn))
            wmap.update({k: fn for k in sh})
        with open(os.path.join(output_dir, "model.safetensors.index.json"), "w") as f:
            json.dump(dict(metadata=dict(total_size=sum(v.numel() * v.element_size() for v in sd.values())), weight_map=wmap), f, indent=1)

    def save_adapter(self, output_dir, base_model_name_or_path=None):
        """peft PeftModel.save_pretrained layout: adapter_model.safetensors + adapter_config.json holding LoraConfig fields only
        (reference utils/common.py:97-98 saves exactly the adapter tensors)."""
        from safetensors.torch import save_file
        os.makedirs(output_dir, exist_ok=True)
        save_file({k: v.contiguous().cpu() for k, v in self.lora_state_dict().items()}, os.path.join(output_dir, "adapter_model.safetensors"))
        lo = self.engine.lora
        cfg = dict(peft_type="LORA", task_type="CAUSAL_LM", base_model_name_or_path=base_model_name_or_path, r=lo["r"],
                   lora_alpha=lo["alpha"], lora_dropout=lo["dropout"], target_modules=list(self.default_lora_target), bias="none",
                   fan_in_fan_out=False, inference_mode=True, modules_to_save=None, init_lora_weights=True)
        with open(os.path.join(output_dir, "adapter_config.json"), "w") as f:
            json.dump(cfg, f, indent=1)

    def load_adapter(self, path):
        from safetensors.torch import load_file
        self.engine.load_lora_state_dict(load_file(os.path.join(path, "adapter_model.safetensors")))

    # ---- LoRA (peft) ---------------------------------------------------------------------------------------
    def apply_lora(self, peft_config):
        """peft.get_peft_model(self, LoraConfig(...)) as the reference's trainer applies it (trl DPOTrainer.__init__ with
        peft_config from utils/auto_load.py:559-571): freezes the base weights, adds adapters on default_lora_target,
        and leaves only lora_A / lora_B trainable.  `peft_config` is a LoraConfig-like object or a dict."""
        get = (lambda k, d=None: peft_config.get(k, d)) if isinstance(peft_config, dict) else (lambda k, d=None: getattr(peft_config, k, d))
        targets = get("target_modules")
        if targets in (None, "auto"):
            targets = self.default_lora_target
        if isinstance(targets, str):
            targets = targets.split(",")
        if sorted(targets) != sorted(self.default_lora_target):
            raise NotImplementedError(f"LoRA target_modules {sorted(targets)}: the MI355X path adapts exactly the decoder "
                                      f"linears {self.default_lora_target} (LlavaForRL.default_lora_target)")
        if get("bias", "none") != "none":
            raise NotImplementedError("lora_bias other than 'none' is not supported on the MI355X path")
        if get("modules_to_save"):
            raise NotImplementedError("modules_to_save is not supported on the MI355X path")
        if not self._trainable:
            raise ValueError("apply_lora needs the trainable policy model")
        self.engine.enable_lora(int(get("r", 64)), float(get("lora_alpha", 16)), float(get("lora_dropout", 0.0) or 0.0),
                                seed=int(get("seed", 0) or 0))
        self.engine.training = self.training
        self._params = nn.ParameterDict()
        self._hf_names = {}
        names = self.engine.lora_layout.hf_names()
        for i, (hf, (k, lo, hi)) in enumerate(names.items()):
            p = nn.Parameter(self.engine.lv[k][lo:hi], requires_grad=True)
            p.grad = self.engine.lgv[k][lo:hi]
            self._params[f"p{i}"] = p
            self._hf_names[f"_params.p{i}"] = hf.replace(".weight", ".default.weight")
        self.peft_config = {"default": peft_config}
        return self

    @property
    def is_packed(self):
        """the decoder projections are GPTQ int4, packed on the device (q_lora)"""
        return self.engine.packed is not None

    @property
    def is_peft_model(self):
        return self.engine.lora is not None and self._trainable

    @contextlib.contextmanager
    def disable_adapter(self):
        """peft PeftModel.disable_adapter(): inside, forwards use the frozen base weights only - trl's null_ref_context
        turns the policy into its own reference model this way."""
        prev = self.engine.lora_active
        self.engine.lora_active = False
        try:
            yield
        finally:
            self.engine.lora_active = prev

    @contextlib.contextmanager
    def reference_pass(self):
        """the trainer's reference forwards run inside: a no-grad forward over a [chosen ; rejected] batch may then compute each pair's
        shared prompt rows once (engine.forward_hidden(prefix_dedup_rows=True)); its log-probs are all anyone reads from such a pass"""
        prev = getattr(self, "_reference_pass", False)
        self._reference_pass = True
        try:
            yield
        finally:
            self._reference_pass = prev

    @contextlib.contextmanager
    def policy_pass(self):
        """the DPO trainer's policy forward runs inside: a training pass over a [chosen ; rejected] batch may then compute each pair's
        shared prompt rows once, forward and backward (engine.forward_hidden(save=True, prefix_dedup_rows=True)).  A no-grad policy
        forward inside it stays dense: only reference_pass() speaks for those."""
        prev = getattr(self, "_policy_pass", False)
        self._policy_pass = True
        try:
            yield
        finally:
            self._policy_pass = prev

    def lora_state_dict(self):
        self.engine.wait_optimizer()
        return self.engine.lora_state_dict()

    def merge_and_unload(self):
        """state dict of the base model with the adapters folded in (peft merge_and_unload); raises on a packed (GPTQ) base, as peft does"""
        return self.engine.merged_weights().state_dict()

    def train(self, mode: bool = True):
        super().train(mode)
        if self._trainable:
            self.engine.training = bool(mode)     # lora_dropout is active in training mode only
        return self

    def create_reference_model(self):
        """trl.create_reference_model: a frozen deep copy of the policy weights sharing the engine (and the frozen ViT)."""
        ref = type(self)(dict(self.engine.cfg), engine=self.engine, weights=self.weights.clone(), trainable=False)
        ref.eval()
        return ref

    # ---- reference wrapper API (docs/CustomizedModel.md:7-11; Llava/__init__.py:273-298) ------------------
    def named_parameters(self, *a, **k):
        for n, p in super().named_parameters(*a, **k):
            if n == "_anchor":
                continue
            yield self._hf_names.get(n, n), p

    def parameters(self, recurse=True):
        for _, p in self.named_parameters():
            yield p

    def state_dict(self, *a, **k):
        self.engine.wait_optimizer()
        out = dict(self.weights.state_dict())
        return out

    @property
    def default_lora_target(self):
        return ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]

    def get_vision_tower(self):
        """the tower this model's forward runs: the trainable one on a policy built with train_vision_tower, else the frozen one"""
        return self.engine.tower if (self.engine.train_vision and self.weights is self.engine.policy) else self.engine.vision

    def freeze_vision_tower(self):
        """reference auto_load.py:554: called unless --freeze_vision_tower False.  Whether the tower trains is decided when the model is
        built (cfg["train_vision_tower"] lays its tensors out in the trainable buffer): a model built to train it cannot be frozen here."""
        if self.engine.train_vision:
            raise ValueError("freeze_vision_tower(): this model was built with train_vision_tower; load it without to keep the tower frozen")
        self._vision_frozen = True

    def gradient_checkpointing_enable(self, gradient_checkpointing_kwargs=None):
        """transformers PreTrainedModel API (the HF Trainer calls it for --gradient_checkpointing True, reference dpo.py:99): the engine
        keeps only each decoder layer's input and re-runs the layer's forward right before its backward - bit-identical results"""
        self.engine.gradient_checkpointing = True

    def gradient_checkpointing_disable(self):
        self.engine.gradient_checkpointing = False

    @property
    def is_gradient_checkpointing(self):
        return bool(self.engine.gradient_checkpointing)

    def prepare_default_generation_kwargs(self, generation_config):
        generation_config.max_new_tokens = 1024
        generation_config.do_sample = False
        return dict(generation_config=generation_config)

    @torch.no_grad()
    def generate(self, input_ids=None, attention_mask=None, max_length=None, max_new_tokens=None, do_sample=False, temperature=None,
                 top_k=None, top_p=None, pad_token_id=None, eos_token_id=None, generation_config=None, generator=None, use_cache=True,
                 merge_lora=True, num_return_sequences=1, sampler=None, repetition_penalty=None, seed=None, output_logprobs=False,
                 sync_every=8, **img):
        """What the reference trainer's `get_batch_samples` calls (base/trainer.py:310-360: `model.generate(input_ids, attention_mask,
        max_length, do_sample=True, pad_token_id, **img_input_dict)`, transformers GenerationMixin defaults: temperature 1, top_k 50,
        top_p 1, use_cache True).  Prompts are LEFT-padded (trl's collator; the merge of the reference end-aligns such rows) and padded
        further to a multiple of 32 tokens.  Finished rows keep receiving `pad_token_id` as in transformers.  Returns prompt +
        continuation ids.

        use_cache=True (engines with supports_kv_cache: LLaVA-1.5, LLaVA-Next): ONE prefill of the prompt fills a per-layer K / V cache
        (engine.forward_hidden(kv_cache=...)), then every new token is one decode step (engine.decode_step: skinny GEMMs and
        split-KV attention over the cache).  The first token's logits are those of the re-forward loop bit for bit (same prefill, same
        lm-head call); later ones differ by the decode kernels' rounding.  With active LoRA adapters:
          merge_lora=True (default, bf16 base): prefill and decode run on the merged weights W + (alpha/r) B A, a second copy of the
            policy computed once per call (peft merge_and_unload);
          merge_lora=False: nothing is merged or cloned - the prefill applies the adapters as every training forward does and each decode
            step runs them live (engine.decode_step -> vlr_decoder_layer_decode_lora), which is what sampling from the policy inside a
            training loop needs; the first token's logits are then those of use_cache=False bit for bit;
          a packed GPTQ base (q_lora) always takes the live path, whatever merge_lora says: nothing can be merged into packed weights.
        With the adapters disabled (disable_adapter()) or absent the plain weights are decoded.  Qwen-VL and InternLM-XComposer2 take
        these routes once the caller has switched their cache on (enable_kv_cache(); a fresh model re-forwards).  use_cache=False, or an
        engine without the cache (Qwen-VL and InternLM-XComposer2 by default): every new token
        re-runs the forward of the whole sequence (the vision features of the batch are cached by the engine), the running batch
        left-padded to a multiple of 32 tokens so that the engine sees a new shape every 32 steps, not every step.

        num_return_sequences = n (also read from generation_config, like do_sample): n samples per prompt; the result has P * n rows, row
        p * n + j being sample j of prompt p (the order of transformers' repeat_interleave expansion).  n > 1 needs do_sample=True
        (transformers refuses greedy search with several return sequences: ValueError).  n == 1 is the code path above, unchanged.
          n > 1 on the KV-cache path (use_cache=True, supports_kv_cache, head_dim 128; all three adapter routes): the P prompts are
            prefilled ONCE into a SharedPromptKVCache, the first logits are repeated n times, and every further token is one decode step
            of P * n rows over the shared prompt K / V plus each sample's own tail (engine.decode_step -> vlr_decoder_layer_decode_shared):
            one prefill, one copy of the prompt's K / V, one read of it per token;
          n > 1 otherwise (use_cache=False, Qwen-VL / InternLM-XComposer2 without enable_kv_cache(), other head dims): ids, mask and every image input are expanded
            by repeat_interleave(n) and the loop above runs on P * n rows - nothing is shared.

        Stop rules of a `generation_config` (each read with getattr(..., None); a call that passes none of them is unchanged):
          eos_token_id (int or list; the keyword wins), pad_token_id (the keyword wins), and stop_words_ids, a list of token-id lists: a
          row is finished once the tokens GENERATED in this call end with one of the sequences (the prompt never counts).  The stop
          tokens stay in the output and later positions receive the pad id, as after an eos.  Both routes and every fan-out check it with
          tensor compares of the last k generated tokens (stop_hit): no host synchronisation beyond the loop's `unfinished.any()`.

        sampler = "torch" (default; also read from generation_config.sampler): the selection above, stock torch ops, temperature 1 /
          top_k 50 / top_p 1 unless the keywords say otherwise (a generation_config's warper settings are NOT read on this path).
        sampler = "device": the selection is one vlr_sample_tokens launch per token (DeviceSampler) on both routes, greedy included.
          temperature / top_k / top_p / repetition_penalty come from the keyword, else from the generation_config, else 1 / 50 / 1 / 1;
          out-of-range values raise ValueError in transformers' words.  repetition_penalty (transformers'
          RepetitionPenaltyLogitsProcessor over the prompt ids, pads included, and the generated ones), seed (None: the generator's
          initial seed, else torch.initial_seed()) and output_logprobs=True (-> (ids, logps [rows][new tokens]), the score transformers'
          compute_transition_scores gives, 0 at pad positions) exist on this path only: with sampler="torch" they raise.  The draw is
          counter-based (seed, self._sampler_calls, row p * n + j, step): the same prompt row draws the same tokens whatever the batch
          around it; self._sampler_calls counts the device-sampled generate calls (save / restore it with a checkpoint).  The host
          reads `unfinished` every sync_every tokens (1 = the per-token cadence); the output does not depend on it."""
        stop_words = None
        if sampler is None:
            sampler = getattr(generation_config, "sampler", None) or "torch"
        if sampler not in ("torch", "device"):
            raise ValueError(f'sampler has to be "torch" or "device", got {sampler!r}')
        if sampler == "torch":
            for name, given in (("repetition_penalty", repetition_penalty is not None and float(repetition_penalty) != 1.0),
                                ("output_logprobs", bool(output_logprobs)), ("seed", seed is not None)):
                if given:
                    raise ValueError(f'{name} needs sampler="device": the torch sampler does not implement it')
        else:
            gc = generation_config
            temperature = temperature if temperature is not None else getattr(gc, "temperature", None)
            top_k = top_k if top_k is not None else getattr(gc, "top_k", None)
            top_p = top_p if top_p is not None else getattr(gc, "top_p", None)
            repetition_penalty = repetition_penalty if repetition_penalty is not None else getattr(gc, "repetition_penalty", None)
        temperature = 1.0 if temperature is None else temperature
        top_k = 50 if top_k is None else top_k
        top_p = 1.0 if top_p is None else top_p
        repetition_penalty = 1.0 if repetition_penalty is None else float(repetition_penalty)
        if sampler == "device":
            if not float(temperature) > 0:
                raise ValueError(f"`temperature` (={temperature}) has to be a strictly positive float, otherwise your next token scores "
                                 "will be invalid.")
            if not 0 < float(top_p) <= 1.0:
                raise ValueError(f"`top_p` has to be a float > 0 and < 1, but is {top_p}")
            if not repetition_penalty > 0:
                raise ValueError(f"`penalty` has to be a strictly positive float, but is {repetition_penalty}")
        if generation_config is not None:
            max_new_tokens = max_new_tokens if max_new_tokens is not None else getattr(generation_config, "max_new_tokens", None)
            do_sample = bool(getattr(generation_config, "do_sample", do_sample))
            use_cache = bool(getattr(generation_config, "use_cache", use_cache))
            nrs = getattr(generation_config, "num_return_sequences", None)
            if nrs is not None and num_return_sequences == 1:
                num_return_sequences = nrs
            if eos_token_id is None:                      # an explicit keyword wins
                eos_token_id = getattr(generation_config, "eos_token_id", None)
            if pad_token_id is None:
                pad_token_id = getattr(generation_config, "pad_token_id", None)
            stop_words = getattr(generation_config, "stop_words_ids", None)
        fanout = int(num_return_sequences)
        if fanout < 1:
            raise ValueError(f"num_return_sequences has to be a positive integer, got {num_return_sequences}")
        if fanout > 1 and not do_sample:
            raise ValueError(f"Greedy methods without beam search do not support num_return_sequences different than 1 (got {fanout}): "
                             "pass do_sample=True")
        if input_ids is None:
            raise ValueError("generate needs input_ids")
        dev = self.engine.dev
        ids = input_ids.to(dev).long()
        mask = (torch.ones_like(ids) if attention_mask is None else attention_mask.to(dev).long())
        B, T0 = ids.shape
        if max_new_tokens is not None:
            limit = T0 + int(max_new_tokens)
        elif max_length is not None:
            limit = int(max_length)
        else:
            limit = T0 + 20                       # transformers' default max_length is 20 NEW tokens when nothing is given
        eos = eos_token_id if eos_token_id is not None else self.config.get("eos_token_id", 2)
        eos = set(eos) if isinstance(eos, (list, tuple)) else {int(eos)}
        pad = int(pad_token_id if pad_token_id is not None else 0)
        stops = stop_sequences(stop_words, dev)
        img = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in img.items()}
        was_training = self.training
        self.eval()
        lm_head = self.weights.v["lm_head"]
        cached = use_cache and getattr(self.engine, "supports_kv_cache", False) and self.engine.hd == 128
        dsamp = None
        if sampler == "device" and T0 >= limit and output_logprobs:      # nothing to generate: the ids as below, and no log-probs
            self.train(was_training)
            return (ids.repeat_interleave(fanout, 0) if fanout > 1 else ids), torch.zeros(B * fanout, 0, dtype=torch.float32, device=dev)
        if sampler == "device" and T0 < limit:
            if seed is None:
                seed = generator.initial_seed() if generator is not None else torch.initial_seed()
            call = getattr(self, "_sampler_calls", 0)
            div = fanout if cached else 1      # the re-forward route expands the prompt rows below: nothing to share
            dsamp = DeviceSampler(ids if div == fanout else ids.repeat_interleave(fanout, 0), div, limit, do_sample, temperature, top_k, top_p,
                                  repetition_penalty, eos, pad, seed, call, stops, sync_every)
            self._sampler_calls = call + 1
        if cached:
            try:        # (fanout / stops / sampler are passed only when set: a call without them is today's call, argument for argument)
                out = self._generate_cached(ids, mask, limit, do_sample, temperature, top_k, top_p, pad, eos, generator, img,
                                            self.cached_lora_route(merge_lora), **({"fanout": fanout} if fanout > 1 else {}),
                                            **({"stops": stops} if stops else {}), **({"sampler": dsamp} if dsamp is not None else {}))
                return dsamp.result(output_logprobs) if dsamp is not None else out
            finally:
                self.train(was_training)
        if fanout > 1:      # no shared cache on this route: the transformers expansion, sample j of prompt p at row p * n + j
            ids, mask = ids.repeat_interleave(fanout, 0), mask.repeat_interleave(fanout, 0)
            img = {k: self._expand_rows(v, B, fanout) for k, v in img.items()}
            B = B * fanout
        if dsamp is not None:
            try:
                return self._generate_reforward_device(dsamp, mask, pad, img, lm_head).result(output_logprobs)
            finally:
                self.train(was_training)
        unfinished = torch.ones(B, dtype=torch.bool, device=dev)
        try:
            while ids.shape[1] < limit and bool(unfinished.any()):
                T = ids.shape[1]
                Tp = (T + 31) // 32 * 32
                if Tp != T:                   # left padding: masked out, and the merged rows stay end-aligned
                    fill = torch.full((B, Tp - T), pad, dtype=ids.dtype, device=dev)
                    run_ids, run_mask = torch.cat([fill, ids], 1), torch.cat([torch.zeros_like(fill), mask], 1)
                else:
                    run_ids, run_mask = ids, mask
                out = self(input_ids=run_ids, attention_mask=run_mask, labels=None, use_cache=False, **img)
                logits = self._last_logits(out.logits.c, B, lm_head)
                if do_sample:
                    nxt = torch.multinomial(sampling_filter(logits, temperature, top_k, top_p).softmax(-1), 1, generator=generator).squeeze(1)
                else:
                    nxt = logits.argmax(-1)
                nxt = torch.where(unfinished, nxt, torch.full_like(nxt, pad))
                ids = torch.cat([ids, nxt[:, None]], 1)
                mask = torch.cat([mask, torch.ones(B, 1, dtype=mask.dtype, device=dev)], 1)
                for e in eos:
                    unfinished = unfinished & (nxt != e)
                if stops:                     # the stop tokens stay in the row; from the next position on it receives the pad id
                    unfinished = unfinished & ~stop_hit(ids[:, T0:], stops)
        finally:
            self.train(was_training)
        return ids

    def _generate_reforward_device(self, ds, mask, pad, img, lm_head):
        """the re-forward loop with the device sampler: the ids grow inside ds.full (the kernel writes each new column), the mask inside a
        buffer allocated once; only the engine's input is assembled per token, as above"""
        dev, B, T = self.engine.dev, ds.rows, ds.T0
        fmask = torch.cat([mask, torch.ones(B, ds.max_new, dtype=mask.dtype, device=dev)], 1)
        while True:
            Tp = (T + 31) // 32 * 32
            if Tp != T:                   # left padding: masked out, and the merged rows stay end-aligned
                fill = torch.full((B, Tp - T), pad, dtype=torch.long, device=dev)
                run_ids, run_mask = torch.cat([fill, ds.full[:, :T]], 1), torch.cat([torch.zeros_like(fill, dtype=fmask.dtype), fmask[:, :T]], 1)
            else:
                run_ids, run_mask = ds.full[:, :T].contiguous(), fmask[:, :T].contiguous()
            out = self(input_ids=run_ids, attention_mask=run_mask, labels=None, use_cache=False, **img)
            ds.select(self._last_logits(out.logits.c, B, lm_head))
            T += 1
            if ds.done():
                return ds

    @staticmethod
    def _expand_rows(v, B, n):
        """an image input of B prompts -> B * n rows in repeat_interleave order (tensors and per-prompt lists; anything else as it is)"""
        if isinstance(v, torch.Tensor) and v.dim() >= 1 and v.shape[0] == B:
            return v.repeat_interleave(n, 0)
        if isinstance(v, (list, tuple)) and len(v) == B:
            return type(v)(x for x in v for _ in range(n))
        return v

    def _last_logits(self, c, B, lm_head):
        """fp32 logits [B][V] of the last attended merged row of every sequence (vlr_gemm_bf16 on at least 8 rows)"""
        dev, H = self.engine.dev, self.engine.H
        S = c["S"]
        valid = c["mask"].view(B, S) != 0
        last = S - 1 - torch.flip(valid, dims=[1]).float().argmax(1)           # last attended position of every row
        rows = max(8, B)
        h_last = torch.zeros(rows, H, dtype=torch.bfloat16, device=dev)
        h_last[:B] = c["hidden"].view(B, S, H)[torch.arange(B, device=dev), last]
        logits = torch.empty(rows, self.engine.V, dtype=torch.float32, device=dev)
        _hip.call("vlr_gemm_bf16", 0, h_last, lm_head, logits, None, None, rows, self.engine.V, H, H, H, self.engine.V, 0, 0, 0, 1)
        return logits[:B]

    def cached_lora_route(self, merge_lora=True):
        """how generate's KV-cache path treats the adapters: "plain" (none, disabled, or a weight set other than the policy), "merged"
        (folded into a clone of the policy once per call) or "live" (un-merged in the prefill and in every decode step: merge_lora=False,
        and always over a packed GPTQ base, into which nothing can be merged)"""
        eng = self.engine
        if not (self.weights is eng.policy and eng.lora is not None and eng.lora_active):
            return "plain"
        return "merged" if (merge_lora and not self.is_packed) else "live"

    def _generate_cached(self, ids, mask, limit, do_sample, temperature, top_k, top_p, pad, eos, generator, img, route, fanout=1, stops=(),
                         sampler=None):
        """generate's KV-cache path: the prefill is the first iteration of the re-forward loop (same padded input, same lm-head
        call) with the K / V rows kept; each further token is one engine.decode_step.  route: cached_lora_route().
        stops: stop_sequences() of the generation config - a row whose generated tokens end with one is finished (stop_hit).
        fanout > 1 (num_return_sequences): the prefill fills the prompt segment of a SharedPromptKVCache, its logits are repeated
        `fanout` times and the B * fanout samples decode over the shared prompt K / V.
        sampler: a DeviceSampler - every selection is its one launch and the caller reads the result from it (None: the torch ops below)."""
        eng, dev = self.engine, self.engine.dev
        B, T = ids.shape
        unfinished = torch.ones(B * fanout, dtype=torch.bool, device=dev)
        if T >= limit:
            return ids.repeat_interleave(fanout, 0) if fanout > 1 else ids
        ws = self.weights
        if ws is eng.policy:
            eng.wait_optimizer()
            if route == "merged":
                ws = eng.merged_weights()          # peft merge: the adapters folded in once for the whole call
        Tp = (T + 31) // 32 * 32
        if Tp != T:                   # left padding: masked out, and the merged rows stay end-aligned
            fill = torch.full((B, Tp - T), pad, dtype=ids.dtype, device=dev)
            run_ids, run_mask = torch.cat([fill, ids], 1), torch.cat([torch.zeros_like(fill), mask], 1)
        else:
            run_ids, run_mask = ids, mask
        pv = img.get("pixel_values")
        if pv is None and not getattr(self, "text_only_prompts", False):      # (Qwen-VL: a prompt may name no image)
            raise ValueError("generate on the MI355X path needs pixel_values")
        if eng.anyres and img.get("image_sizes") is None:
            raise ValueError("LLaVA-Next generate needs image_sizes (reference LlavaNext/__init__.py:216-222)")
        cache = eng.new_kv_cache(B, limit - T) if fanout == 1 else eng.new_shared_kv_cache(B, fanout, limit - T)
        c = eng.forward_hidden(ws, run_ids, run_mask, None, pv, image_dup=int(getattr(pv, "_vlr_dup", 1)), save=False,
                               tag="policy_ng" if self.weights is eng.policy else "ref", image_sizes=img.get("image_sizes"),
                               kv_cache=cache if fanout == 1 else cache.prompt)
        logits = self._last_logits(c, B, ws.v["lm_head"])
        out = [ids]
        if fanout > 1:
            cache.begin()
            logits = logits.repeat_interleave(fanout, 0)
            out = [ids.repeat_interleave(fanout, 0)]
        n = T
        if sampler is not None:
            while True:
                nxt = sampler.select(logits)
                if sampler.done():
                    return sampler.full
                logits = eng.decode_step(ws, nxt, cache)
        if stops:
            keep = max(s.numel() for s in stops)
            tail = torch.empty(B * fanout, 0, dtype=torch.long, device=dev)
        while True:
            if do_sample:
                nxt = torch.multinomial(sampling_filter(logits, temperature, top_k, top_p).softmax(-1), 1, generator=generator).squeeze(1)
            else:
                nxt = logits.argmax(-1)
            nxt = torch.where(unfinished, nxt, torch.full_like(nxt, pad))
            out.append(nxt[:, None].to(ids.dtype))
            n += 1
            for e in eos:
                unfinished = unfinished & (nxt != e)
            if stops:                         # the last tokens GENERATED so far (never the prompt's) against every stop sequence
                tail = torch.cat([tail, nxt[:, None]], 1)[:, -keep:]
                unfinished = unfinished & ~stop_hit(tail, stops)
            if n >= limit or not bool(unfinished.any()):
                break
            logits = eng.decode_step(ws, nxt, cache)
        return torch.cat(out, 1)

    def zero_grad(self, set_to_none: bool = True):
        self.engine.zero_grad()

    def prefetch_vision(self, img_input_dict):
        pv = img_input_dict.get("pixel_values")
        if pv is not None:
            dup = getattr(pv, "_vlr_dup", 1)
            self.engine.vision_features(pv[: pv.shape[0] // dup] if dup > 1 else pv)

    def get_input_embeddings(self):
        return self.weights.v["embed"]

    # ---- causal-LM loss (SFT) ---------------------------------------------------------------------------
    ce_selects_by_mask = True      # reference Llava :246-257 / LlavaNext :322-331: rows with shifted merged attention mask != 0

    def _loss_fn(self, logits, c):
        """the reference's `loss` of forward(labels=...), deferred: CrossEntropyLoss (ignore_index -100) over the shifted positions - for
        the LLaVA wrappers those the shifted MERGED attention mask keeps, for Qwen-VL / InternLM-XComposer2 (ce_selects_by_mask False)
        every position; the label alone decides there (modeling_qwen.py:839-842, InternLMXC2/__init__.py:211-219)."""
        def fn():
            sel = c["mask"].view(c["Bn"], c["S"])[:, 1:].ne(0).to(torch.uint8).contiguous() if self.ce_selects_by_mask else None
            return logits.cross_entropy(c["labels"], sel, -100)
        return fn

    @staticmethod
    def causal_lm_loss(outputs):
        """the scalar the reference returns as `outputs.loss` (computed on this call if it has not been read yet)"""
        return outputs.loss

    # ---- forward ----------------------------------------------------------------------------------------
    def forward(self, input_ids=None, pixel_values=None, attention_mask=None, position_ids=None, past_key_values=None,
                inputs_embeds=None, vision_feature_layer=None, vision_feature_select_strategy=None, labels=None,
                use_cache=None, output_attentions=None, output_hidden_states=None, return_dict=None, image_sizes=None):
        """reference Llava/__init__.py:111-271 on the training path.  Returns `logits` (lazy), the EXPANDED `labels`
        and `image_position_map`; the reference's cross-entropy `loss` (:246-257) is computed when it is first read (SFT), never on the DPO path."""
        if inputs_embeds is not None or past_key_values is not None or use_cache:
            raise NotImplementedError("generation / KV-cache inputs are outside the MI355X DPO training path")
        if pixel_values is None:
            raise ValueError("LlavaForRL.forward on the DPO path needs pixel_values")
        if vision_feature_layer not in (None, -2) or vision_feature_select_strategy not in (None, "default"):
            raise ValueError(f"Unexpected select feature strategy: {vision_feature_select_strategy}")
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        dup = int(getattr(pixel_values, "_vlr_dup", 1))
        grad = torch.is_grad_enabled() and self._trainable and self.training
        if self.engine.anyres and image_sizes is None:
            raise ValueError("LLaVA-Next forward needs image_sizes (reference LlavaNext/__init__.py:216-222)")
        if grad:
            hidden = _HiddenFn.apply(self._anchor, self, input_ids, attention_mask, labels, pixel_values, dup, image_sizes)
            c = self._last_ctx
        else:
            c = self.engine.forward_hidden(self.weights, input_ids, attention_mask, labels, pixel_values, image_dup=dup,
                                           save=False, tag="policy_ng" if self.weights is self.engine.policy else "ref",
                                           image_sizes=image_sizes, prefix_dedup_rows=bool(getattr(self, "_reference_pass", False)))
            hidden = c["hidden"]
        out_labels = c["labels"] if labels is not None else torch.full_like(c["mask"], -100, dtype=torch.long)
        if c.get("meta") is not None:
            out_labels._vlr_meta = c["meta"]          # per-batch host-side facts (trainer.concatenated_inputs)
        logits = LazyLogits(self.engine, c, hidden)
        return LlavaRLOutputWithPast(loss=None, logits=logits, labels=out_labels, image_position_map=c["img_map"],
                                     loss_fn=self._loss_fn(logits, c) if labels is not None else None)


# ----------------------------------------------------------------------------------------------------------
class LlavaProcessor(VLProcessor):
    def __init__(self, model_name_or_path=None, tokenizer=None, image_processor=None, **kwargs) -> None:
        if model_name_or_path is not None:
            import transformers
            self.processor = transformers.LlavaProcessor.from_pretrained(model_name_or_path, **kwargs)
            self._tok, self._ip = self.processor.tokenizer, self.processor.image_processor
        else:
            self.processor = None
            self._tok, self._ip = tokenizer, image_processor

    @property
    def tokenizer(self):
        return self._tok

    @property
    def chat_template(self):
        return VLChatTemplate(system_begin=None, system_end=None, user_begin="USER: ", user_end="",
                              assistant_begin="ASSISTANT: ", assistant_end="", image_placeholder="<image>\n")

    @property
    def image_processor(self):
        return self._ip

    def save_pretrained(self, output_dir):
        if self.processor is not None:
            return self.processor.save_pretrained(output_dir)

    def process_batch_conv(self, sources, system_message=None, add_end_for_empty_value=False):
        """reference Llava/__init__.py:343-388."""
        if not isinstance(sources, list) or not isinstance(sources[0], list):
            raise ValueError("sources must be a batch of conversations, eg. List[List[Dict]]")
        t = self.chat_template
        begin = {"user": t.user_begin, "assistant": t.assistant_begin}
        end = {"user": t.user_end, "assistant": t.assistant_end}
        raw_texts, b_ids, b_masks, b_labels = [], [], [], []
        for source in sources:
            raw, labels, prev = "", [], 0
            ids, masks = [], []
            for i, s in enumerate(source):
                raw += begin[s["from"]] + s["value"] + (end[s["from"]] if s["value"] != "" or add_end_for_empty_value else "")
                text_tokens = self.tokenizer(s["value"], padding=False, add_special_tokens=(i == 0))
                cur = self.tokenizer(raw)
                ids, masks = cur["input_ids"], cur["attention_mask"]
                ext = len(ids) - prev
                prev = len(ids)
                labels.extend([-100] * ext)
                if s["from"] == "assistant" and len(text_tokens["input_ids"]) != 0:
                    n = min(ext, len(text_tokens["input_ids"]), len(labels))
                    labels[-n:] = text_tokens["input_ids"][-n:]
            labels = [l if m == 1 else -100 for l, m in zip(labels, masks)]
            assert len(ids) == len(masks) == len(labels), f"input_ids:{len(ids)}, attention_masks:{len(masks)}, labels:{len(labels)}"
            b_ids.append(ids)
            b_masks.append(masks)
            b_labels.append(labels)
            raw_texts.append(raw)
        return {"prompt": None, "answer": None,
                "full": dict(input_ids=b_ids, attention_mask=b_masks, labels=b_labels), "raw_str": raw_texts}

    @staticmethod
    def format_multimodal_prompt(prompt: str, img_paths=None):
        if img_paths is None:
            return prompt
        if not isinstance(img_paths, list):
            img_paths = [img_paths]
        if len(img_paths) == 1 and "<image>" not in prompt:
            return "<image>\n" + prompt
        assert prompt.count("<image>") == len(img_paths), \
            f"The number of given image ({len(img_paths)}) does not match the number of image placeholders in the prompt: {prompt}"
        return prompt.replace("<image>", "<image>\n")

    @staticmethod
    def remove_image_placeholder(prompt: str):
        return prompt.replace("<image>\n", "")

    @staticmethod
    def is_multimodal_prompt_valid(prompt: str):
        return "<image>\n" in prompt

    def train(self):
        self.tokenizer.pad_token = self.tokenizer.unk_token

    def infer(self):
        self.tokenizer.pad_token = self.tokenizer.bos_token

    def __call__(self, texts=None, convs=None, images_path=None, padding=True, padding_side="left", check_format=True):
        inputs = super().__call__(texts, convs, images_path, padding, padding_side, check_format)
        if images_path is not None:
            inputs["pixel_values"] = load_pixel_values(flatten_list(images_path), self.image_processor)
        return inputs


CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def load_pixel_values(items, image_processor=None) -> torch.Tensor:
    """paths / PIL images -> CLIP-normalised fp32 [n,3,S,S] via the HF CLIPImageProcessor (reference :435-443); items that
    already are [3,S,S] float tensors (synthetic data) pass through."""
    if all(isinstance(i, torch.Tensor) for i in items):
        return torch.stack([i.float() for i in items])
    from PIL import Image
    imgs = [Image.open(i).convert("RGB") if isinstance(i, str) else i for i in items]
    return image_processor(images=imgs, return_tensors="pt")["pixel_values"]


@dataclass
class LlavaDPODataCollatorWithPadding(VLDPODataCollatorWithPadding):
    def __call__(self, features: List[Dict[str, Any]]) -> Dict[str, Any]:
        padded = super().__call__(features)
        ip = self.processor.image_processor if self.processor is not None else None
        padded["img_input_dict"] = dict(pixel_values=load_pixel_values(padded["img_path"], ip))
        return padded


class LlavaDPOTrainer(VLDPOTrainer):
    ...


@dataclass
class LlavaSFTDataCollatorWithPadding(VLSFTDataCollatorWithPadding):
    def __call__(self, features: List[Dict[str, Any]]) -> Dict[str, Any]:
        """reference :447-453: pixel_values at the top level of the batch, img_path dropped"""
        padded = super().__call__(features)
        ip = self.processor.image_processor if self.processor is not None else None
        padded["pixel_values"] = load_pixel_values(padded.pop("img_path"), ip)
        return padded


class LlavaSFTTRainer(VLSFTTrainer):          # sic: the reference's spelling (:483)
    ...


class LlavaForRM(LlavaForRL):
    """LlavaForRL whose engine carries the reward head in its trainable buffers (cfg["rm_head"]): the base model of LlavaRewardModel"""

    def __init__(self, cfg: dict, **kw):
        super().__init__(dict(cfg, rm_head=True), **kw)


class LlavaRewardModel(VLRewardModel):
    """reference Llava/__init__.py LlavaRewardModel: reward = rm_head at merged column T - 1 + images * (P - 1)"""
    base_cls = LlavaForRM
    image_count_key = "image_token"


@dataclass
class LlavaRMDataCollatorWithPadding(VLRMDataCollatorWithPadding):
    def __call__(self, features: List[Dict[str, Any]]) -> Dict[str, Any]:
        padded = super().__call__(features)
        ip = self.processor.image_processor if self.processor is not None else None
        padded["img_input_dict"] = dict(pixel_values=load_pixel_values(padded["img_path"], ip))
        return padded


class LlavaRMTrainer(VLRMTrainer):
    ...


class LlavaForPPO(LlavaForRL):
    """LlavaForRL whose engine carries the PPO value head in its trainable buffers (cfg["v_head"]): the base model of LlavaWithValueHead"""

    def __init__(self, cfg: dict, **kw):
        super().__init__(dict(cfg, v_head=True), **kw)


class LlavaWithValueHead(VLModelWithValueHead):
    """reference Llava/__init__.py LlavaWithValueHead: the policy of PPO, v_head.summary on every position's final hidden state"""
    base_cls = LlavaForPPO
    image_count_key = "image_token"


@dataclass
class LlavaPPODataCollator(VLPPODataCollator):
    def __call__(self, features: List[Dict[str, Any]]) -> Dict[str, Any]:
        """reference :466-471: the rows' images as `pixel_values` [n, 3, s, s]"""
        batch = super().__call__(features)
        ip = self.processor.image_processor if self.processor is not None else None
        batch["pixel_values"] = load_pixel_values(flatten_list(batch["img_path"]), ip)
        return batch


class LlavaPPOTrainer(VLPPOTrainer):
    ...


# The PPO record of this package.  ModelCoreMapper's value_model / ppo_collator / ppo_trainer slots stay None (models/utils.py says why).
ppo_core = PPOCore(value_model=LlavaWithValueHead, collator=LlavaPPODataCollator, trainer=LlavaPPOTrainer)


class LlavaGRPOTrainer(VLGRPOTrainer):
    ...


# The GRPO record: the policy is the plain wrapper, the queries are collated as PPO's are.
grpo_core = GRPOCore(model=LlavaForRL, collator=LlavaPPODataCollator, trainer=LlavaGRPOTrainer)


class LlavaKTOTrainer(VLKTOTrainer):
    dpo_trainer_cls = LlavaDPOTrainer      # prompt + one answer are tokenised as this family's DPO trainer tokenises them


# The KTO record: the rows are collated by the DPO collator (base/collator.py VLKTODataCollatorWithPadding wraps it).
kto_core = KTOCore(dpo_collator=LlavaDPODataCollatorWithPadding, trainer=LlavaKTOTrainer)


core_mapper = ModelCoreMapper(
    model=LlavaForRL,
    processor=LlavaProcessor,
    dpo_collator=LlavaDPODataCollatorWithPadding,
    dpo_trainer=LlavaDPOTrainer,
    reward_model=LlavaRewardModel,
    reward_collator=LlavaRMDataCollatorWithPadding,
    reward_trainer=LlavaRMTrainer,
    sft_collator=LlavaSFTDataCollatorWithPadding,
    sft_trainer=LlavaSFTTRainer,
)
