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
