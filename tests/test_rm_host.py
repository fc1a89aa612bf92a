"""CPU-only checks of the reward-model path: the collator against torch's pad_sequence, the argument parsing of vlrlhf.reward_modeling,
the registry slots, the two new library exports and their argument errors, the flat layouts with and without the reward head, and the
rm_head.bin round trip of the wrapper's host side.  The reward fixtures' shape facts and the oracle's reward values are pinned here too:
the GPU tests (tests/test_hip_rm.py) rely on them."""
import hashlib
import json
import os
from types import SimpleNamespace

import pytest
import torch
from torch.nn.utils.rnn import pad_sequence

from tests import rm_ref as R
from tests.golden_util import load_case

FAMILY = {"llava_hipsmall": None, "qwenvl_small": "qwen_vl", "llavanext_small": None, "internlmxc2_small": "internlm_xc2"}
# ParamLayout (numel, n_decay, n_opt, offsets) and LoraLayout(r=8) (numel, offsets) of the four committed fixtures' configs as they were
# before the reward head existed; offsets as sha256(json(sorted(offset.items())))[:16]
LAYOUTS_BEFORE = {
    "llava_hipsmall": (402304, 401408, 402304, "2c81d5def176de8c", 34816, "f4999e61e276b9db"),
    "qwenvl_small": (1508096, 1504512, 1508096, "738b505e95914fa0", 40960, "f7784bad658a109a"),
    "llavanext_small": (985088, 983296, 985088, "dd482d6a690858bb", 53248, "eef07696e1a4c0f4"),
    "internlmxc2_small": (2430720, 2331904, 2331904, "d69f2564f01177bc", 45056, "79c62269e57dfd40"),
}


def _cfg(case):
    cfg = load_case(case)[1]
    return dict(cfg, family=FAMILY[case]) if FAMILY[case] else cfg


def _sig(layout):
    return hashlib.sha256(json.dumps(sorted(layout.offset.items())).encode()).hexdigest()[:16]


# ------------------------------------------------------------------------------------------------------------ collator
def test_rm_collator_matches_pad_sequence_and_refuses_stray_keys():
    from vlrlhf.base.collator import VLRMDataCollatorWithPadding
    g = torch.Generator().manual_seed(0)
    rows = []
    for n_c, n_r in ((5, 9), (11, 3), (1, 9)):
        rows.append(dict(input_ids_chosen=torch.randint(1, 50, (n_c,), generator=g).tolist(), attention_mask_chosen=[1] * n_c,
                         input_ids_rejected=torch.randint(1, 50, (n_r,), generator=g).tolist(), attention_mask_rejected=[1] * n_r,
                         img_path=f"{n_c}.jpg"))
    got = VLRMDataCollatorWithPadding(pad_token_id=7)(rows)
    for k, pad in (("input_ids_chosen", 7), ("attention_mask_chosen", 0), ("input_ids_rejected", 7), ("attention_mask_rejected", 0)):
        exp = pad_sequence([torch.LongTensor(r[k]) for r in rows], batch_first=True, padding_value=pad)
        assert got[k].dtype == torch.long and torch.equal(got[k], exp), k
    assert got["input_ids_chosen"].shape == (3, 11) and got["input_ids_rejected"].shape == (3, 9)      # each side to its own width
    assert got["img_path"] == ["5.jpg", "11.jpg", "1.jpg"]
    with pytest.raises(ValueError, match="Unexpected key in batch 'labels_chosen'"):
        VLRMDataCollatorWithPadding(pad_token_id=0)([dict(rows[0], labels_chosen=[1])])


def test_family_collators_build_img_input_dict():
    from vlrlhf.models.Llava import LlavaRMDataCollatorWithPadding
    from vlrlhf.models.QwenVL import QwenVLRMDataCollatorWithPadding
    px = torch.arange(3 * 4 * 4, dtype=torch.float32).view(3, 4, 4)
    row = dict(input_ids_chosen=[1, 2], attention_mask_chosen=[1, 1], input_ids_rejected=[3], attention_mask_rejected=[1], img_path=px)
    for cls in (LlavaRMDataCollatorWithPadding, QwenVLRMDataCollatorWithPadding):
        out = cls(pad_token_id=0)([row, row])
        assert torch.equal(out["img_input_dict"]["pixel_values"], torch.stack([px, px])), cls.__name__


# ------------------------------------------------------------------------------------------------------------ entry point
def test_reward_modeling_arguments():
    from vlrlhf import reward_modeling as rm
    s, t, l = rm._parse(rm.ScriptArguments, rm.TrainingArguments, rm.LoraArguments, argv=[])
    assert l.modules_to_save == "rm_head" and l.lora_r == 64 and l.lora_dropout == 0.05 and l.q_lora is False
    assert s.score_margin == -1 and s.max_length == 512 and s.freeze_vision_tower is True and s.data_dir is None
    assert s.model_name_or_path == "llava-hf/llava-1.5-7b-hf" and t.group_name == "Qwen-VL-Chat-rm" and t.use_lora is False
    s, t, l = rm._parse(rm.ScriptArguments, rm.TrainingArguments, rm.LoraArguments,
                        argv=["--data_dir", "/d", "--score_margin", "2.5", "--max_length", "64", "--use_lora", "True", "--lora_r", "8",
                              "--modules_to_save", "rm_head", "--learning_rate", "1e-5", "--gradient_checkpointing", "True"])
    assert s.data_dir == "/d" and s.score_margin == 2.5 and s.max_length == 64 and t.use_lora and t.learning_rate == 1e-5
    model = SimpleNamespace(base_model=SimpleNamespace(default_lora_target=["q_proj", "v_proj"]))
    cfg = rm.lora_config_from_args(model, t, l)
    assert cfg["modules_to_save"] == ["rm_head"] and cfg["r"] == 8 and cfg["target_modules"] == ["q_proj", "v_proj"]
    assert rm.lora_config_from_args(model, SimpleNamespace(use_lora=False), l) is None
    l.q_lora = True
    with pytest.raises(NotImplementedError, match="q_lora"):
        rm.lora_config_from_args(model, t, l)


# ------------------------------------------------------------------------------------------------------------ registry
def test_registry_reward_slots(tmp_path):
    from vlrlhf.base.collator import VLRMDataCollatorWithPadding
    from vlrlhf.base.model import VLRewardModel
    from vlrlhf.base.trainer import VLRMTrainer
    from vlrlhf.utils import auto_load as A
    for arch, filled in (("LlavaForConditionalGeneration", True), ("QWenLMHeadModel", True), ("LlavaNextForConditionalGeneration", False),
                         ("InternLMXComposer2ForCausalLM", False)):
        cm = A.auto_core_mapper(arch)
        slots = (cm.reward_model, cm.reward_collator, cm.reward_trainer)
        if filled:
            assert issubclass(slots[0], VLRewardModel) and issubclass(slots[1], VLRMDataCollatorWithPadding) and issubclass(slots[2], VLRMTrainer)
            assert slots[0].base_cls is not None and issubclass(slots[0].base_cls, cm.model)
        else:
            assert slots == (None, None, None)
        assert cm.value_model is None and cm.ppo_collator is None and cm.ppo_trainer is None
        d = tmp_path / arch
        d.mkdir()
        (d / "config.json").write_text(json.dumps(dict(architectures=[arch])))
        if filled:
            assert isinstance(A.MyAutoRMCollator(str(d), pad_token_id=3), cm.reward_collator)
        else:
            for call in (lambda: A.MyAutoRewardModel.from_pretrained(str(d)), lambda: A.MyAutoRMCollator(str(d)), lambda: A.MyAutoRMTrainer(str(d))):
                with pytest.raises(NotImplementedError, match=r"Llava.*QwenVL"):
                    call()


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_rm_exports_and_argument_errors_without_gpu():
    from vlrlhf import _hip
    l = _hip.lib()
    assert hasattr(l, "vlr_rm_head_fwd") and hasattr(l, "vlr_rm_head_bwd")
    assert "vlr_rm_head_fwd" in _hip.exported_symbols() and "vlr_rm_head_bwd" in _hip.exported_symbols()
    assert _hip.helper("vlr_abi_version") == 9                  # additive entry points: no caller breaks
    assert l.vlr_rm_head_fwd(None, 8, None, None, None, None, 1, 8, None) == 1 and b"vlr_rm_head_fwd" in l.vlr_last_error()
    assert l.vlr_rm_head_bwd(None, 8, None, None, None, None, 8, None, None, 0, 1, 8, None) == 1 and b"vlr_rm_head_bwd" in l.vlr_last_error()
    # shapes are refused before anything is launched: H below 8 / not a multiple of 8, a row stride below H, no rows
    p = torch.zeros(64, dtype=torch.float32).data_ptr()
    for n, H, ld in ((1, 4, 8), (1, 12, 16), (1, 16, 8), (0, 8, 8)):
        assert l.vlr_rm_head_fwd(p, ld, p, p, p, p, n, H, None) == 1 and b"bad shape" in l.vlr_last_error(), (n, H, ld)
        assert l.vlr_rm_head_bwd(p, ld, p, p, p, p, ld, p, p, 0, n, H, None) == 1 and b"bad shape" in l.vlr_last_error(), (n, H, ld)


# ------------------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("case", sorted(LAYOUTS_BEFORE))
def test_layouts_without_rm_head_are_unchanged(case):
    from vlrlhf.engine import LoraLayout, ParamLayout
    cfg = _cfg(case)
    p, lo = ParamLayout(cfg), LoraLayout(cfg, 8)
    assert (p.numel, p.n_decay, p.n_opt, _sig(p), lo.numel, _sig(lo)) == LAYOUTS_BEFORE[case]
    assert "rm_head.w" not in p.offset and "rm_head.w" not in lo.offset and lo.n_decay == lo.numel
    assert ParamLayout(dict(cfg, rm_head=False)).offset == p.offset


@pytest.mark.parametrize("case", ["llava_hipsmall", "qwenvl_small"])
def test_layouts_with_rm_head_add_two_entries(case):
    from vlrlhf.engine import LoraLayout, ParamLayout
    cfg = _cfg(case)
    H = cfg["hidden"]
    p0, p1 = ParamLayout(cfg), ParamLayout(dict(cfg, rm_head=True))
    assert set(p1.offset) - set(p0.offset) == {"rm_head.w", "rm_head.b"} and set(p0.offset) <= set(p1.offset)
    assert p1.shape["rm_head.w"] == (H,) and p1.shape["rm_head.b"] == (1,)
    assert [n for n, _, _ in p1.entries if not n.startswith("rm_head.")] == [n for n, _, _ in p0.entries]      # the order of the rest stands
    w, b = p1.offset["rm_head.w"], p1.offset["rm_head.b"]
    assert w + H <= p1.n_decay and w == p0.n_decay                    # the weight closes the decay region
    assert p1.n_decay <= b < p1.n_opt and b + 8 == p1.n_opt == p1.numel - (p0.numel - p0.n_opt)      # the bias closes the no-decay region
    assert p1.numel == p0.numel + H + 8 and p1.n_decay == p0.n_decay + H
    assert p1.bucket_after["tail"] == (p0.bucket_after["tail"][0], p1.n_opt)      # the DDP tail bucket covers both
    assert {k: v for k, v in p1.bucket_after.items() if k != "tail"} == {k: v for k, v in p0.bucket_after.items() if k != "tail"}
    assert all(".b" in n or "ln" in n or n == "norm" for n, o in p1.offset.items() if p1.n_decay <= o < p1.n_opt)
    assert not any(hf is None for hf, *_ in p1.hf_names()) and len(list(p1.hf_names())) == len(list(p0.hf_names()))      # not a checkpoint tensor
    l0, l1 = LoraLayout(cfg, 8), LoraLayout(dict(cfg, rm_head=True), 8)
    assert set(l1.offset) - set(l0.offset) == {"rm_head.w", "rm_head.b"}
    assert {k: l1.offset[k] for k in l0.offset} == l0.offset
    assert l1.offset["rm_head.w"] == l0.numel and l1.n_decay == l0.numel + H == l1.offset["rm_head.b"] and l1.numel == l1.n_decay + 8
    assert l1.hf_names() == l0.hf_names()                            # the adapter file keeps the names save_adapter writes today


# ------------------------------------------------------------------------------------------------------------ rm_head.bin
class _HostEngine:
    """the three engine calls VLRewardModel's host side makes, on CPU tensors"""

    def __init__(self, H):
        self.H, self.cfg = H, dict(rm_head=True)
        self.w, self.b = torch.zeros(H, dtype=torch.bfloat16), torch.zeros(1, dtype=torch.bfloat16)
        self.gw, self.gb = torch.zeros_like(self.w), torch.zeros_like(self.b)

    def rm_head_views(self):
        return self.w, self.b, self.gw, self.gb

    def set_rm_head(self, weight, bias):
        self.w.copy_(weight.reshape(-1).to(torch.bfloat16))
        self.b.copy_(bias.reshape(-1).to(torch.bfloat16))

    def wait_optimizer(self):
        pass


class _HostBase(torch.nn.Module):
    is_peft_model = False

    def __init__(self, H):
        super().__init__()
        self.engine, self.config, self.saved = _HostEngine(H), {}, []

    def save_pretrained(self, d, *a, **k):
        os.makedirs(d, exist_ok=True)
        self.saved.append(d)


def test_rm_head_bin_round_trip_on_the_host(tmp_path):
    from vlrlhf.base.model import VLRewardModel, init_rm_head, load_rm_head
    H = 136
    w0, b0 = init_rm_head(H, seed=3)
    assert w0.shape == (1, H) and float(w0.abs().max()) <= 1 / H ** 0.5 and float(b0) == 0.0 and w0.std() > 0.3 / H ** 0.5
    assert torch.equal(init_rm_head(H, seed=3)[0], w0) and not torch.equal(init_rm_head(H, seed=4)[0], w0)
    m = VLRewardModel(_HostBase(H), seed=3)
    assert torch.equal(m.rm_head.weight.detach(), w0.bfloat16()) and m.rm_head.weight.shape == (1, H) and m.rm_head.bias.shape == (1,)
    assert m.rm_head.weight.data_ptr() == m.engine.w.data_ptr() and m.rm_head.weight.grad.data_ptr() == m.engine.gw.data_ptr()
    w, b = R.rm_head(H)
    m.engine.set_rm_head(w, b)
    out = str(tmp_path / "out")
    m.save_pretrained(out)
    assert m.base_model.saved == [out]
    sd = torch.load(os.path.join(out, "rm_head.bin"))
    assert set(sd) == {"weight", "bias"} and sd["weight"].shape == (1, H) and sd["bias"].shape == (1,)
    lin = torch.nn.Linear(H, 1)
    lin.load_state_dict(sd)                                            # what the reference's loader does with the file
    assert torch.equal(lin.weight.detach(), w.bfloat16().float().view(1, H)) and float(lin.bias) == 0.25
    m2 = VLRewardModel(_HostBase(H), load_rm_head(out))
    assert torch.equal(m2.engine.w, m.engine.w) and torch.equal(m2.engine.b, m.engine.b)
    assert load_rm_head(str(tmp_path)) is None                        # no file: a base model, the head is freshly initialised
    m3 = VLRewardModel(_HostBase(H), load_rm_head(str(tmp_path)), seed=3)
    assert torch.equal(m3.engine.w, w0.bfloat16().view(-1))
    assert [n for n, _ in m.named_parameters()] == ["rm_head.weight", "rm_head.bias"]
    with pytest.raises(ValueError, match="rm_head"):
        base = _HostBase(H)
        base.engine.cfg = {}
        VLRewardModel(base)


def test_apply_lora_accepts_only_the_reward_head_in_modules_to_save():
    from vlrlhf.base.model import VLRewardModel
    seen = []

    class Base(_HostBase):
        def apply_lora(self, cfg):
            seen.append(cfg)

    m = VLRewardModel(Base(8))
    for mts in (None, ["rm_head"], "rm_head"):
        m.apply_lora(dict(r=8, lora_alpha=16, modules_to_save=mts))
        assert "modules_to_save" not in seen[-1] and seen[-1]["r"] == 8      # the base wrapper keeps refusing modules_to_save: it gets none
    for mts in (["lm_head"], ["rm_head", "lm_head"], "embed_tokens"):
        with pytest.raises(NotImplementedError, match="modules_to_save"):
            m.apply_lora(SimpleNamespace(r=8, lora_alpha=16, modules_to_save=mts))
    assert len(seen) == 3


# ------------------------------------------------------------------------------------------------------------ fixtures + oracle
ORACLE = {   # fp32 oracle on each half alone, head of rm_ref.rm_head(H) with the bias taken off: (r_chosen, r_rejected, loss)
    "llava_hipsmall": ([-0.6826, 0.2242], [-0.3853, 0.3712], 0.81105),
    "qwenvl_small": ([0.6942, 0.6193], [-0.5020, 0.2766], 0.40027),
}


@pytest.mark.parametrize("case,widths", [("llava_hipsmall", (42, 50)), ("qwenvl_small", (40, 37))])
def test_reward_fixtures_and_oracle_values(case, widths):
    z, cfg, W, W_ref, batch, rows = load_case(case)
    rb = R.rm_batch(batch)
    extra = 0 if "visual" in cfg else (cfg["image_size"] // cfg["patch_size"]) ** 2 - 1
    assert (rb["input_ids_chosen"].shape[1] + extra, rb["input_ids_rejected"].shape[1] + extra) == widths      # halves of different width
    last = torch.cat([rb["attention_mask_chosen"][:, -1], rb["attention_mask_rejected"][:, -1]])
    assert bool((last == 0).any()) and bool((last == 1).any())      # rewards read at padding rows AND at real tokens
    w, b = R.rm_head(cfg["hidden"])
    rc, rr = R.rewards(W, cfg, rb, w, b)
    exp_c, exp_r, exp_loss = ORACLE[case]
    assert torch.allclose(rc - R.HEAD_BIAS, torch.tensor(exp_c), atol=1e-4) and torch.allclose(rr - R.HEAD_BIAS, torch.tensor(exp_r), atol=1e-4)
    assert abs(float(R.pair_loss(rc, rr)) - exp_loss) < 1e-5


def test_oracle_loss_falls_over_eight_steps():
    """what the GPU trajectory test relies on: the oracle loop (fixture optimizer settings, full fine-tune) brings the loss down"""
    from oracle import llava_dpo_oracle as O
    z, cfg, W, W_ref, batch, rows = load_case("llava_hipsmall")
    w, b = R.rm_head(cfg["hidden"])
    losses = R.train_loop(W, cfg, R.rm_batch(batch), w, b, cfg["optim"], 8, emulate=O.HIP_ROUNDING)
    assert all(b_ < a_ for a_, b_ in zip(losses, losses[1:])) and losses[-1] < 0.5 * losses[0], losses
