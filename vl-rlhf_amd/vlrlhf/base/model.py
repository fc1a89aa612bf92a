"""Reward model for MI355X - mirror of the reference src/vlrlhf/base/model.py:12-69 (VLRewardModel): a base model wrapper plus
`rm_head = nn.Linear(hidden, 1)`, reward = rm_head(hidden_states[-1][:, -1, :]) - the post-final-norm hidden state at the LAST COLUMN
of the padded batch, a padding row for every sequence shorter than its batch (reference behaviour, kept).

The head lives in the engine's trainable flat buffer (cfg["rm_head"]: vlrlhf.engine.ParamLayout / LoraLayout), so clip, AdamW, the DDP
buckets and the optimizer checkpoint cover it; the arithmetic is vlr_rm_head_fwd / vlr_rm_head_bwd (include/vlr.h).  Deliberate
differences: rewards are fp32 (the reference's are bf16, the dtype of the model); the lm-head never runs - the reference adds
0.0 * mean(logits) to the hidden states, which changes no value and gives the lm-head a zero gradient, reproduced by the engine
(reward_backward) without the GEMM."""
import math
import os

import torch
import torch.nn as nn


class _RewardFn(torch.autograd.Function):
    """hidden [M, H] -> rewards [n] fp32 at `rows` (engine.reward_forward / reward_backward) as one autograd node"""

    @staticmethod
    def forward(ctx, hidden, engine, c, rows):
        rewards, lp = engine.reward_forward(c, rows)
        ctx.lp, ctx.engine = lp, engine
        return rewards

    @staticmethod
    def backward(ctx, d_rewards):
        dh = ctx.engine.reward_backward(ctx.lp, d_rewards.contiguous())
        ctx.lp = None
        return dh, None, None, None


def init_rm_head(hidden_size: int, seed: int = 0):
    """nn.Linear(hidden, 1) as the reference builds it: weight ~ kaiming_uniform(a=sqrt(5)) = U(-1/sqrt(H), 1/sqrt(H)), bias 0 -
    drawn on the host from `seed` (the training seed), so every rank starts from the same head"""
    g = torch.Generator().manual_seed(int(seed))
    bound = 1.0 / math.sqrt(hidden_size)
    return (torch.rand(1, hidden_size, generator=g) * 2 - 1) * bound, torch.zeros(1)


def load_rm_head(path: str):
    """rm_head.bin of `path` -> (weight [1, H], bias [1]) or None when the directory has none (a base model)"""
    fn = os.path.join(path, "rm_head.bin")
    if not os.path.exists(fn):
        return None
    sd = torch.load(fn, map_location="cpu")
    return sd["weight"], sd["bias"]


class VLRewardModel(nn.Module):
    base_cls = None            # the base wrapper with cfg["rm_head"] switched on (LlavaRewardModel / QwenVLRewardModel set it)
    image_count_key = "image_token"      # engine cfg key of the id that marks one image in input_ids

    def __init__(self, base_model, rm_head=None, seed: int = 0):
        super().__init__()
        if not base_model.engine.cfg.get("rm_head"):
            raise ValueError("VLRewardModel needs a base model whose engine was built with cfg['rm_head'] (use from_pretrained / "
                             "from_state_dict of the reward-model class)")
        self.base_model = base_model
        self.config = base_model.config
        w, b = rm_head if rm_head is not None else init_rm_head(base_model.engine.H, seed)
        base_model.engine.set_rm_head(w, b)
        self._bind_head()

    def _bind_head(self):
        """the head's nn.Parameters = views of the engine's flat buffers (gradients included), as the base wrapper's are"""
        w, b, gw, gb = self.engine.rm_head_views()
        self.rm_head = nn.Module()
        self.rm_head.weight = nn.Parameter(w.view(1, -1), requires_grad=True)
        self.rm_head.bias = nn.Parameter(b, requires_grad=True)
        self.rm_head.weight.grad, self.rm_head.bias.grad = gw.view(1, -1), gb

    # ---- construction -------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, cfg: dict, sd, rm_head=None, seed: int = 0):
        return cls(cls.base_cls.from_state_dict(cfg, sd), rm_head, seed)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *args, seed: int = 0, **kwargs):
        """the base wrapper's from_pretrained + rm_head.bin of the same directory; without that file the head is freshly initialised
        from `seed` (reference _get_reward_head_from_pretrained).  GPTQ checkpoints (q_lora) are refused: the reward head over a packed
        base has not been exercised."""
        base = cls.base_cls.from_pretrained(pretrained_model_name_or_path, *args, **kwargs)
        if base.is_packed:
            raise NotImplementedError("reward modelling over GPTQ int4 base weights (q_lora) is not supported on the MI355X path")
        return cls(base, load_rm_head(pretrained_model_name_or_path), seed)

    def rm_head_state_dict(self):
        """{"weight": [1, H], "bias": [1]} - what nn.Linear(hidden, 1).state_dict() holds (bf16, the dtype of the model)"""
        self.engine.wait_optimizer()
        w, b, _, _ = self.engine.rm_head_views()
        return {"weight": w.detach().view(1, -1).cpu().clone(), "bias": b.detach().cpu().clone()}

    def save_pretrained(self, save_directory, *args, **kwargs):
        """the base model through its own save_pretrained - under LoRA the adapter, under the names save_adapter writes - plus
        rm_head.bin next to it"""
        if self.is_peft_model:
            return self.save_adapter(save_directory)
        self.base_model.save_pretrained(save_directory, *args, **kwargs)
        torch.save(self.rm_head_state_dict(), os.path.join(save_directory, "rm_head.bin"))

    def save_adapter(self, output_dir, base_model_name_or_path=None):
        self.base_model.save_adapter(output_dir, base_model_name_or_path=base_model_name_or_path)
        torch.save(self.rm_head_state_dict(), os.path.join(output_dir, "rm_head.bin"))

    def load_adapter(self, path):
        self.base_model.load_adapter(path)
        self.load_rm_head(path)

    def load_rm_head(self, path):
        head = load_rm_head(path)
        if head is not None:
            self.engine.set_rm_head(*head)
        return head is not None

    # ---- peft ---------------------------------------------------------------------------------------------
    def apply_lora(self, peft_config):
        """get_peft_model(model, LoraConfig(..., modules_to_save=["rm_head"])): adapters on the base wrapper's default targets, and the
        head stays trainable - it is trained whether modules_to_save names it or not (nothing else can be named)."""
        get = (lambda k, d=None: peft_config.get(k, d)) if isinstance(peft_config, dict) else (lambda k, d=None: getattr(peft_config, k, d))
        mts = get("modules_to_save")
        if isinstance(mts, str):
            mts = mts.split(",")
        if mts not in (None, [], ["rm_head"], ("rm_head",)):
            raise NotImplementedError(f"modules_to_save={mts}: the MI355X reward model keeps exactly the reward head trainable "
                                      "beside the adapters (None or ['rm_head'])")
        inner = {k: get(k) for k in ("r", "lora_alpha", "lora_dropout", "target_modules", "bias", "task_type", "seed") if get(k) is not None}
        self.base_model.apply_lora(inner)
        self.base_model.peft_config = {"default": peft_config}
        self._bind_head()
        return self

    @property
    def is_peft_model(self):
        return self.base_model.is_peft_model

    @property
    def engine(self):
        return self.base_model.engine

    def gradient_checkpointing_enable(self, *args, **kwargs):
        return self.base_model.gradient_checkpointing_enable(*args, **kwargs)

    def named_parameters(self, *a, **k):
        for n, p in self.base_model.named_parameters():
            yield "base_model." + n, p
        yield "rm_head.weight", self.rm_head.weight
        yield "rm_head.bias", self.rm_head.bias

    def parameters(self, recurse=True):
        for _, p in self.named_parameters():
            yield p

    def zero_grad(self, set_to_none: bool = True):
        self.engine.zero_grad()

    # ---- forward ------------------------------------------------------------------------------------------
    def _image_counts(self, input_ids):
        """images per row; every row of a batch must carry the same number, or a row's last column is not where the rule below puts it"""
        meta = getattr(input_ids, "_vlr_meta", None)
        if meta is not None and "rm_images" in meta:
            return meta["rm_images"]
        cnt = (input_ids == int(self.engine.cfg[self.image_count_key])).sum(-1)
        lo, hi = int(cnt.min()), int(cnt.max())
        if lo != hi:
            raise ValueError(f"reward model: the rows of a batch must carry the same number of images, got between {lo} and {hi}")
        if meta is not None:
            meta["rm_images"] = lo
        return lo

    def reward_rows(self, c, input_ids, reward_cols=None):
        """dense row index b * S + column of every sequence's reward.  reward_cols [Bn] names the column in TOKEN space (None: the last
        column of input_ids, the reference's `-1`); the merged column is that plus what the image tokens in front of it expanded by -
        S - T when every row carries the same number of images, which forward checks (LLaVA: images * (P - 1); Qwen-VL: 0, its slots are
        tokens)."""
        Bn, T, S = c["Bn"], c["T"], c["S"]
        dev = self.engine.dev
        if reward_cols is None:
            cols = torch.full((Bn,), T - 1, dtype=torch.int64, device=dev)
        else:
            cols = torch.as_tensor(reward_cols, dtype=torch.int64).to(dev)
            if cols.numel() != Bn or int(cols.min()) < 0 or int(cols.max()) >= T:
                raise ValueError(f"reward_cols must name one column in [0, {T}) per sequence ({Bn}), got {cols.tolist()}")
        return (torch.arange(Bn, device=dev, dtype=torch.int64) * S + cols + (S - T)).to(torch.int32)

    def forward(self, input_ids, attention_mask, reward_cols=None, **kwargs):
        """-> (rewards [Bn, 1] fp32,) - a tuple, as the reference returns for trl RewardTrainer.compute_loss.  `reward_cols`: the
        trainer's concatenated [chosen ; rejected] pass names each half's own last column."""
        for k in ("labels", "output_hidden_states", "return_dict", "use_cache"):
            kwargs.pop(k, None)
        self._image_counts(input_ids)
        out = self.base_model(input_ids=input_ids, attention_mask=attention_mask, labels=None, **kwargs)
        lg = out.logits
        c, hidden = lg.c, lg.hidden
        rows = self.reward_rows(c, input_ids, reward_cols)
        if hidden.requires_grad:
            rewards = _RewardFn.apply(hidden, self.engine, c, rows)
        else:
            rewards, _ = self.engine.reward_forward(c, rows)
        return (rewards.unsqueeze(-1),)

    @torch.no_grad()
    def score(self, input_ids, attention_mask, **kwargs):
        """forward under no_grad in eval mode, for callers that rank samples (generate(num_return_sequences=n)); -> rewards [Bn] fp32"""
        was_training = self.training
        self.eval()
        try:
            return self.forward(input_ids, attention_mask, **kwargs)[0].squeeze(-1)
        finally:
            self.train(was_training)


# ------------------------------------------------------------------------------------------------------------------------------------
# PPO policy with a value head - mirror of the reference src/vlrlhf/base/model.py VLModelWithValueHead (trl 0.8.1
# AutoModelForCausalLMWithValueHead over a base wrapper): v_head.summary = nn.Linear(hidden, 1) on the final hidden state of EVERY position.
# The PPO step reads log-probs and values only where the logits predict a response token, so forward(labels=...) returns both compact, on
# the R response rows of vlr_build_rows, through ONE autograd node; the head lives in the engine's trainable flat buffer (cfg["v_head"]),
# exactly as the reward head does.  Deliberate differences: no value-head dropout (trl's summary_dropout_prob: the rollout and the
# optimisation passes must see the same values, and the reference recipe sets none); values are fp32; the [B, S, V] logits are the
# engine's lazy stand-in, never a tensor.
# ------------------------------------------------------------------------------------------------------------------------------------
V_HEAD_KEYS = ("v_head.summary.weight", "v_head.summary.bias")


class _PpoHeadsFn(torch.autograd.Function):
    """hidden [M, H] -> (token log-probs [R], values [R]) on the response rows (engine.ppo_forward / ppo_backward) as one autograd node"""

    @staticmethod
    def forward(ctx, hidden, model, c, labels, label_pad, entropy=False):
        tok, values, lp = model.engine.ppo_forward(c, labels, label_pad, entropy)      # (the entropy is a statistic: read from lp, no gradient)
        ctx.lp, ctx.engine = lp, model.engine
        model._last_lp = lp
        return tok, values

    @staticmethod
    def backward(ctx, dlogp, dvalues):
        R = ctx.lp["R"]
        zero = lambda: torch.zeros(R, dtype=torch.float32, device=ctx.engine.dev)      # noqa: E731
        dh = ctx.engine.ppo_backward(ctx.lp, zero() if dlogp is None else dlogp.contiguous(), zero() if dvalues is None else dvalues.contiguous())
        ctx.lp = None
        return dh, None, None, None, None, None


class _TokenLogpsFn(torch.autograd.Function):
    """hidden [M, H] -> token log-probs [R] on the response rows (engine.token_logps_forward / token_logps_backward) as one autograd node"""

    @staticmethod
    def forward(ctx, hidden, model, c, labels, label_pad):
        tok, lp = model.engine.token_logps_forward(c, labels, label_pad)
        ctx.lp, ctx.engine = lp, model.engine
        model._last_lp = lp
        return tok

    @staticmethod
    def backward(ctx, dlogp):
        dh = ctx.engine.token_logps_backward(ctx.lp, dlogp.contiguous())
        ctx.lp = None
        return dh, None, None, None, None


class _TokenLogpsEntFn(torch.autograd.Function):
    """hidden [M, H] -> (token log-probs [R], policy entropy [R]) on the response rows as one autograd node: the lm-head pass with the
    entropy in its epilogue.  An entropy output that receives no gradient costs nothing in the backward (the existing lm-head backward
    runs); one that does hands d entropy to the entropy backward."""

    @staticmethod
    def forward(ctx, hidden, model, c, labels, label_pad):
        tok, lp = model.engine.token_logps_forward(c, labels, label_pad, entropy=True)
        ctx.lp, ctx.engine = lp, model.engine
        ctx.set_materialize_grads(False)
        model._last_lp = lp
        return tok, lp["entropy"]

    @staticmethod
    def backward(ctx, dlogp, dent):
        if dlogp is None:
            dlogp = torch.zeros(ctx.lp["R"], dtype=torch.float32, device=ctx.engine.dev)
        dh = ctx.engine.token_logps_backward(ctx.lp, dlogp.contiguous(), None if dent is None else dent.contiguous())
        ctx.lp = None
        return dh, None, None, None, None


def token_logps(model, input_ids, attention_mask, labels, return_entropy=False, **img):
    """-> token log-probs [R] fp32 of a PLAIN family wrapper (LlavaForRL, QwenVLForRL: no value head) on the R response rows - the
    positions whose logits predict a token with label != -100, sequence after sequence; token_seq_off(model) [Bn + 1] delimits them.
    What GRPO trains on: the same forward as VLModelWithValueHead's, without the value head.  return_entropy: -> (log-probs, entropy
    [R] fp32 of each row's softmax over the vocabulary) from the same lm-head pass; the log-probs keep their bits and the entropy is
    differentiable."""
    if labels is None:
        raise ValueError("token_logps needs labels (-100 outside the response): log-probs exist on the response rows only")
    out = model(input_ids=input_ids, attention_mask=attention_mask, labels=labels, **img)
    lg = out.logits
    c, hidden = lg.c, lg.hidden
    if hidden.requires_grad:
        return (_TokenLogpsEntFn if return_entropy else _TokenLogpsFn).apply(hidden, model, c, c["labels"], -100)
    tok, model._last_lp = model.engine.token_logps_forward(c, c["labels"], -100, entropy=return_entropy)
    return (tok, model._last_lp["entropy"]) if return_entropy else tok


def token_seq_off(model):
    """[Bn + 1] int32 on the device: the rows of sequence b in the last token_logps(model, ...) are seq_off[b] .. seq_off[b + 1]"""
    lp = getattr(model, "_last_lp", None)
    if lp is None:
        raise RuntimeError("token_seq_off: no token_logps(model, ...) has run yet")
    return lp["seq_off"]


def init_v_head(hidden_size: int, strategy=None, initializer_range: float = 0.2, seed: int = 0):
    """trl ValueHead + _init_weights: `None` keeps nn.Linear's default (weight and bias ~ U(-1/sqrt(H), 1/sqrt(H))), "normal" draws the
    weight from N(0, initializer_range) and zeroes the bias - on the host from `seed`, so every rank starts from the same head"""
    g = torch.Generator().manual_seed(int(seed))
    if strategy is None:
        bound = 1.0 / math.sqrt(hidden_size)
        return (torch.rand(1, hidden_size, generator=g) * 2 - 1) * bound, (torch.rand(1, generator=g) * 2 - 1) * bound
    if strategy == "normal":
        return torch.randn(1, hidden_size, generator=g) * float(initializer_range), torch.zeros(1)
    raise ValueError(f"v_head_init_strategy must be None or 'normal', got {strategy!r}")


def load_v_head(path: str):
    """the two v_head.summary.* tensors of `path`: v_head.bin (full fine-tune) or pytorch_model.bin (LoRA, reference common.py:113-117)
    -> (weight, bias), or None when the directory has neither (a base model)"""
    for fn in ("v_head.bin", "pytorch_model.bin"):
        f = os.path.join(path, fn)
        if os.path.exists(f):
            sd = torch.load(f, map_location="cpu")
            if all(k in sd for k in V_HEAD_KEYS):
                return sd[V_HEAD_KEYS[0]], sd[V_HEAD_KEYS[1]]
    return None


class VLModelWithValueHead(nn.Module):
    base_cls = None            # the base wrapper with cfg["v_head"] switched on (LlavaWithValueHead / QwenVLWithValueHead set it)
    image_count_key = "image_token"      # engine cfg key of the id that marks one image in input_ids (the trainer cuts image inputs by it)

    def __init__(self, base_model, v_head=None, v_head_init_strategy=None, v_head_initializer_range: float = 0.2, seed: int = 0, **kwargs):
        super().__init__()
        self._refuse(kwargs)
        if not base_model.engine.cfg.get("v_head"):
            raise ValueError("VLModelWithValueHead needs a base model whose engine was built with cfg['v_head'] (use from_pretrained / "
                             "from_state_dict of the value-head class)")
        self.pretrained_model = base_model
        self.config = base_model.config
        w, b = v_head if v_head is not None else init_v_head(base_model.engine.H, v_head_init_strategy, v_head_initializer_range, seed)
        base_model.engine.set_v_head(w, b)
        self._last_lp = None
        self._bind_head()

    @staticmethod
    def _refuse(kwargs):
        """what the reference's class takes and this one does not build: named errors instead of a silently different model"""
        if kwargs.pop("use_value_adapter", False):
            raise NotImplementedError("use_value_adapter: a value adapter on a shared base is not built on the MI355X path; the value head "
                                      "reads the policy's own hidden states")
        if kwargs.pop("reward_adapter", None) is not None:
            raise NotImplementedError("reward_adapter: a reward adapter on the policy's base is not built on the MI355X path; score with a "
                                      "separate reward model (VLRewardModel.score)")
        kwargs.pop("summary_dropout_prob", None)      # trl's value-head dropout: deliberately not applied
        if kwargs:
            raise TypeError(f"VLModelWithValueHead: unexpected arguments {sorted(kwargs)}")

    def compute_reward_score(self, *args, **kwargs):
        raise NotImplementedError("compute_reward_score needs a reward_adapter on the policy's base, which the MI355X path does not build; "
                                  "score with a separate reward model (VLRewardModel.score)")

    def _bind_head(self):
        """the head's nn.Parameters = views of the engine's flat buffers (gradients included), as the base wrapper's are"""
        w, b, gw, gb = self.engine.v_head_views()
        self.v_head = nn.Module()
        self.v_head.summary = nn.Module()
        self.v_head.summary.weight = nn.Parameter(w.view(1, -1), requires_grad=True)
        self.v_head.summary.bias = nn.Parameter(b, requires_grad=True)
        self.v_head.summary.weight.grad, self.v_head.summary.bias.grad = gw.view(1, -1), gb

    # ---- construction -------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, cfg: dict, sd, v_head=None, **kwargs):
        return cls(cls.base_cls.from_state_dict(cfg, sd), v_head, **kwargs)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *args, v_head_init_strategy=None, v_head_initializer_range: float = 0.2,
                        seed: int = 0, use_value_adapter=False, reward_adapter=None, summary_dropout_prob=None, **kwargs):
        """the base wrapper's from_pretrained + the value head of the same directory (v_head.bin or pytorch_model.bin); without one the
        head is freshly initialised.  GPTQ checkpoints (q_lora) are refused: the value head over a packed base has not been exercised."""
        cls._refuse(dict(use_value_adapter=use_value_adapter, reward_adapter=reward_adapter))
        base = cls.base_cls.from_pretrained(pretrained_model_name_or_path, *args, **kwargs)
        if base.is_packed:
            raise NotImplementedError("PPO over GPTQ int4 base weights (q_lora) is not supported on the MI355X path")
        return cls(base, load_v_head(pretrained_model_name_or_path), v_head_init_strategy, v_head_initializer_range, seed)

    def v_head_state_dict(self):
        """exactly the two keys trl's state_dict adds: v_head.summary.weight [1, H], v_head.summary.bias [1] (bf16, the dtype of the model)"""
        self.engine.wait_optimizer()
        w, b, _, _ = self.engine.v_head_views()
        return {V_HEAD_KEYS[0]: w.detach().view(1, -1).cpu().clone(), V_HEAD_KEYS[1]: b.detach().cpu().clone()}

    def save_pretrained(self, save_directory, *args, **kwargs):
        """full fine-tune: the base checkpoint + v_head.bin; LoRA: the adapter files + pytorch_model.bin holding exactly the two
        v_head.summary.* keys (reference utils/common.py:113-117)"""
        if self.is_peft_model:
            return self.save_adapter(save_directory)
        self.pretrained_model.save_pretrained(save_directory, *args, **kwargs)
        torch.save(self.v_head_state_dict(), os.path.join(save_directory, "v_head.bin"))

    def save_adapter(self, output_dir, base_model_name_or_path=None):
        self.pretrained_model.save_adapter(output_dir, base_model_name_or_path=base_model_name_or_path)
        torch.save(self.v_head_state_dict(), os.path.join(output_dir, "pytorch_model.bin"))

    def load_adapter(self, path):
        self.pretrained_model.load_adapter(path)
        self.load_v_head(path)

    def load_v_head(self, path):
        head = load_v_head(path)
        if head is not None:
            self.engine.set_v_head(*head)
        return head is not None

    # ---- peft ---------------------------------------------------------------------------------------------
    def apply_lora(self, peft_config):
        """adapters on the base wrapper's default targets; the value head stays trainable beside them (trl keeps v_head outside peft)"""
        get = (lambda k, d=None: peft_config.get(k, d)) if isinstance(peft_config, dict) else (lambda k, d=None: getattr(peft_config, k, d))
        mts = get("modules_to_save")
        if isinstance(mts, str):
            mts = mts.split(",")
        if mts not in (None, [], ["v_head"], ("v_head",)):
            raise NotImplementedError(f"modules_to_save={mts}: the MI355X PPO policy keeps exactly the value head trainable beside the "
                                      "adapters (None or ['v_head'])")
        inner = {k: get(k) for k in ("r", "lora_alpha", "lora_dropout", "target_modules", "bias", "task_type", "seed") if get(k) is not None}
        self.pretrained_model.apply_lora(inner)
        self.pretrained_model.peft_config = {"default": peft_config}
        self._bind_head()
        return self

    @property
    def is_peft_model(self):
        return self.pretrained_model.is_peft_model

    @property
    def engine(self):
        return self.pretrained_model.engine

    def gradient_checkpointing_enable(self, *args, **kwargs):
        return self.pretrained_model.gradient_checkpointing_enable(*args, **kwargs)

    def disable_adapter(self):
        return self.pretrained_model.disable_adapter()

    def generate(self, *args, **kwargs):
        return self.pretrained_model.generate(*args, **kwargs)

    def named_parameters(self, *a, **k):
        for n, p in self.pretrained_model.named_parameters():
            yield "pretrained_model." + n, p
        yield V_HEAD_KEYS[0], self.v_head.summary.weight
        yield V_HEAD_KEYS[1], self.v_head.summary.bias

    def parameters(self, recurse=True):
        for _, p in self.named_parameters():
            yield p

    def zero_grad(self, set_to_none: bool = True):
        self.engine.zero_grad()

    # ---- forward ------------------------------------------------------------------------------------------
    def forward(self, input_ids, attention_mask=None, labels=None, return_logits=False, return_entropy=False, **kwargs):
        """-> (token log-probs [R] fp32, None, values [R] fp32) on the R response rows: the positions whose logits predict a token with
        label != -100 (trl reads logprobs and values[:, :-1] under the same mask), sequence after sequence - `self.seq_off` [Bn + 1]
        delimits them.  The middle element is trl's `loss`, never computed.  return_logits=True puts the lazy [B, S, V] logits stand-in of
        the base wrapper in the first slot instead (values still need labels).  return_entropy=True appends the policy entropy [R] fp32
        of the same rows (a statistic, detached: PPO has no entropy term), from the same lm-head pass."""
        for k in ("output_hidden_states", "return_dict", "use_cache", "past_key_values"):
            kwargs.pop(k, None)
        if labels is None and not return_logits:
            raise ValueError("VLModelWithValueHead.forward needs labels (-100 outside the response): log-probs and values exist on the "
                             "response rows only; pass return_logits=True for the lazy [B, S, V] logits")
        out = self.pretrained_model(input_ids=input_ids, attention_mask=attention_mask, labels=labels, **kwargs)
        lg = out.logits
        if labels is None:
            return lg, None, None
        c, hidden = lg.c, lg.hidden
        if hidden.requires_grad:
            tok, values = _PpoHeadsFn.apply(hidden, self, c, c["labels"], -100, bool(return_entropy))
        else:
            tok, values, self._last_lp = self.engine.ppo_forward(c, c["labels"], -100, bool(return_entropy))
        if return_entropy:
            return (lg if return_logits else tok), None, values, self._last_lp["entropy"]
        return (lg if return_logits else tok), None, values

    @property
    def seq_off(self):
        """[Bn + 1] int32 on the device: the rows of sequence b in the last forward's compact outputs are seq_off[b] .. seq_off[b + 1]"""
        if self._last_lp is None:
            raise RuntimeError("seq_off: no forward(labels=...) has run yet")
        return self._last_lp["seq_off"]
