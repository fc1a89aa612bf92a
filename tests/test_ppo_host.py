"""PPO without a GPU: the checker's own arithmetic (tests/ppo_ref.py) on hand-computed cases, the argument rules of PPOConfig, the KL
controllers, the refusals of the value-head model, the PPO registry record beside the untouched ModelCoreMapper slots, the engine layouts
with the value head, the exports and argument errors of the three new entry points, tokenize_row and the collators on the tiny
processor, and the arguments, rules and refusals of vlrlhf/ppo.py."""
import math

import pytest
import torch

from tests import ppo_ref as PR
from tests.golden_util import load_case


# ------------------------------------------------------------------------------------------------------------ the checker, by hand
def test_gae_by_hand():
    adv, ret = PR.gae(torch.tensor([0.0, 0.0, 1.0]).double(), torch.tensor([0.5, 0.5, 0.5]).double(), [0, 3], 1.0, 0.5)
    assert adv.tolist() == [0.125, 0.25, 0.5] and ret.tolist() == [0.625, 0.75, 1.0]
    # two sequences: nothing crosses the boundary, V past the end of EACH sequence is 0
    adv, ret = PR.gae(torch.tensor([0.0, 1.0, 2.0]).double(), torch.ones(3).double(), [0, 2, 3], 0.5, 1.0)
    assert adv.tolist() == [-0.5, 0.0, 1.0] and ret.tolist() == [0.5, 1.0, 2.0]
    # a sequence of one token
    adv, _ = PR.gae(torch.tensor([3.0]).double(), torch.tensor([1.0]).double(), [0, 1], 0.9, 0.9)
    assert adv.tolist() == [2.0]


def test_masked_whiten_by_hand():
    x = torch.tensor([1.0, 2.0, 3.0, 4.0]).double()
    sd = math.sqrt(1.25 * 4 / 3 + 1e-8)                      # biased variance 1.25, times R / (R - 1)
    y = PR.masked_whiten(x)
    assert torch.allclose(y, torch.tensor([-1.5, -0.5, 0.5, 1.5]).double() / sd, rtol=0, atol=1e-15)
    assert torch.allclose(PR.masked_whiten(x, shift_mean=False), y + 2.5, rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="at least 2"):
        PR.masked_whiten(torch.tensor([1.0]))


def test_rewards_by_hand():
    old, ref = torch.tensor([-1.0, -2.0, -1.0]).double(), torch.tensor([-1.5, -1.0, -1.0]).double()
    assert PR.kl_penalty(old, ref, "kl").tolist() == [0.5, -1.0, 0.0]
    assert PR.kl_penalty(old, ref, "abs").tolist() == [0.5, 1.0, 0.0]
    assert PR.kl_penalty(old, ref, "mse").tolist() == [0.125, 0.5, 0.0]
    with pytest.raises(NotImplementedError, match="full"):
        PR.kl_penalty(old, ref, "full")
    r, nsr, kl = PR.rewards(old, ref, [0, 2, 3], torch.tensor([2.0, -1.0]).double(), 0.1, "kl")
    assert torch.allclose(nsr, torch.tensor([-0.05, 0.1, 0.0]).double()) and torch.allclose(r, torch.tensor([-0.05, 2.1, -1.0]).double())
    out = PR.advantages(old.float(), ref.float(), torch.zeros(3), [0, 2, 3], torch.tensor([2.0, -1.0]), 0.1, "kl", 1.0, 1.0, False)
    assert torch.allclose(out["kl_sums"], torch.tensor([-0.5, 0.0]).double()) and abs(float(out["stats"][0]) + 0.25) < 1e-12
    assert torch.allclose(out["returns"], torch.tensor([2.05, 2.1, -1.0]).double())       # gamma = lam = 1, V = 0: the rewards to go
    assert abs(float(out["advantages"].mean())) < 1e-12


def test_loss_by_hand_ties_and_threshold():
    logp = torch.tensor([-1.0, -2.0])
    args = (logp, torch.tensor([1.0, 0.0]), logp.clone(), torch.tensor([1.0, 0.0]), torch.tensor([1.0, -2.0]), torch.tensor([0.0, 1.0]))
    st, dlogp, dvpred = PR.loss_and_grads(*args, 0.2, 0.2, 0.1, 10.0)
    # ratio = 1 sits inside the clip range, vpred = V_old inside its own: max() ties, clamp passes - the unclipped derivatives
    assert st["pg"] == 0.5 and st["vf"] == 0.5 and abs(st["loss"] - 0.55) < 1e-15 and st["ratio"] == 1.0 and st["skipped"] == 0.0
    assert dlogp.tolist() == [-0.5, 1.0] and torch.allclose(dvpred, torch.tensor([0.05, -0.05]).double())
    assert st["pg_clipfrac"] == 0.0 and st["vf_clipfrac"] == 0.0 and st["approxkl"] == 0.0 and st["policykl"] == 0.0
    st, dlogp, dvpred = PR.loss_and_grads(*args, 0.0, 0.0, 0.1, 10.0)                      # clip range 0: the bounds ARE the values, still passed
    assert dlogp.tolist() == [-0.5, 1.0] and torch.allclose(dvpred, torch.tensor([0.05, -0.05]).double())
    st, dlogp, dvpred = PR.loss_and_grads(*args, 0.2, 0.2, 0.1, 0.5, upstream=0.5)         # mean ratio 1 > 0.5: everything exactly 0
    assert st["skipped"] == 1.0 and st["loss"] == 0.0 and st["pg"] == 0.0 and st["vf"] == 0.0
    assert dlogp.abs().sum() == 0 and dvpred.abs().sum() == 0 and st["error"] == 1.0
    _, dlogp, _ = PR.loss_and_grads(*args, 0.2, 0.2, 0.1, 10.0, upstream=0.5)
    assert dlogp.tolist() == [-0.25, 0.5]


def test_kl_controllers():
    from vlrlhf.base.trainer import AdaptiveKLController, FixedKLController
    for mod in (PR, None):
        A, F = (mod.AdaptiveKLController, mod.FixedKLController) if mod else (AdaptiveKLController, FixedKLController)
        c = A(0.2, 6.0, 100.0)
        c.update(9.0, 2)                                     # kl / target - 1 = 0.5 -> clipped to 0.2
        assert abs(c.value - 0.2 * (1 + 0.2 * 2 / 100)) < 1e-15
        c.update(3.0, 2)                                     # -0.5 -> -0.2
        assert abs(c.value - 0.2 * (1 + 0.2 * 2 / 100) * (1 - 0.2 * 2 / 100)) < 1e-15
        c.update(6.3, 2)                                     # inside the clip
        assert abs(c.value - 0.2 * 1.004 * 0.996 * (1 + 0.05 * 2 / 100)) < 1e-12
        f = F(0.2)
        f.update(100.0, 2)
        assert f.value == 0.2


# ------------------------------------------------------------------------------------------------------------ config, refusals, registry
def test_ppo_config_rules():
    from vlrlhf.base.trainer import PPOConfig
    c = PPOConfig(batch_size=8, mini_batch_size=2, gradient_accumulation_steps=2)
    assert c.backward_batch_size == 4 and c.ppo_epochs == 4 and c.lam == 0.95 and c.gamma == 1.0 and c.max_grad_norm is None
    assert (c.cliprange, c.cliprange_value, c.vf_coef, c.init_kl_coef, c.target, c.horizon, c.ratio_threshold) == (0.2, 0.2, 0.1, 0.2, 6.0, 10000.0, 10.0)
    for bad in (dict(batch_size=6, mini_batch_size=4), dict(batch_size=8, mini_batch_size=4, gradient_accumulation_steps=3), dict(batch_size=0)):
        with pytest.raises(ValueError, match="multiple"):
            PPOConfig(**bad)
    with pytest.raises(ValueError, match="kl_penalty"):
        PPOConfig(batch_size=2, mini_batch_size=2, kl_penalty="js")


def test_value_head_model_refusals_and_init():
    from vlrlhf.base.model import VLModelWithValueHead, init_v_head
    with pytest.raises(NotImplementedError, match="use_value_adapter"):
        VLModelWithValueHead._refuse(dict(use_value_adapter=True))
    with pytest.raises(NotImplementedError, match="reward_adapter"):
        VLModelWithValueHead._refuse(dict(reward_adapter="some/adapter"))
    with pytest.raises(TypeError, match="unexpected"):
        VLModelWithValueHead._refuse(dict(bogus=1))
    VLModelWithValueHead._refuse(dict(use_value_adapter=False, reward_adapter=None, summary_dropout_prob=0.1))      # the dropout is dropped, by design
    w, b = init_v_head(64, "normal", 0.2, seed=3)
    w2, _ = init_v_head(64, "normal", 0.2, seed=3)
    assert w.shape == (1, 64) and torch.equal(w, w2) and float(b) == 0.0
    w, b = init_v_head(64, None, seed=3)                     # nn.Linear's default: both within 1 / sqrt(H)
    assert float(w.abs().max()) <= 0.125 and abs(float(b)) <= 0.125 and float(b) != 0.0
    with pytest.raises(ValueError, match="v_head_init_strategy"):
        init_v_head(64, "xavier")


def test_ppo_registry_and_untouched_mapper_slots():
    from vlrlhf.base.model import VLModelWithValueHead
    from vlrlhf.base.trainer import VLPPOTrainer
    from vlrlhf.models import InternLMXC2, Llava, LlavaNext, QwenVL
    from vlrlhf.utils import auto_load
    assert auto_load.PPO_FAMILIES == ["Llava", "QwenVL"]
    for arch, pkg in (("LlavaForConditionalGeneration", Llava), ("QWenLMHeadModel", QwenVL)):
        vm, tr = auto_load._ppo_slot(arch, "value_model"), auto_load._ppo_slot(arch, "trainer")
        assert vm is pkg.ppo_core.value_model and issubclass(vm, VLModelWithValueHead) and issubclass(tr, VLPPOTrainer)
        assert vm.base_cls.__mro__[1] is pkg.core_mapper.model
        from vlrlhf.base.collator import VLPPODataCollator
        assert issubclass(auto_load._ppo_slot(arch, "collator"), VLPPODataCollator) and pkg.ppo_core.collator is auto_load._ppo_slot(arch, "collator")
    for arch in ("LlavaNextForConditionalGeneration", "InternLMXComposer2ForCausalLM"):
        with pytest.raises(NotImplementedError, match="LLaVA-1.5 and Qwen-VL"):
            auto_load._ppo_slot(arch, "value_model")
    for pkg in (Llava, LlavaNext, QwenVL, InternLMXC2):      # the record's three PPO slots stay as the reward-model tests pin them
        m = pkg.core_mapper
        assert m.value_model is None and m.ppo_collator is None and m.ppo_trainer is None
    assert not hasattr(LlavaNext, "ppo_core") and not hasattr(InternLMXC2, "ppo_core")


# ------------------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("case", ["llava_hipsmall", "qwenvl_small"])
def test_layouts_with_v_head_add_two_entries(case):
    from vlrlhf.engine import LoraLayout, ParamLayout
    cfg = load_case(case)[1]
    H = cfg["hidden"]
    p0, p1 = ParamLayout(cfg), ParamLayout(dict(cfg, v_head=True))
    assert ParamLayout(dict(cfg, v_head=False)).offset == p0.offset
    assert set(p1.offset) - set(p0.offset) == {"v_head.w", "v_head.b"}
    assert [n for n, _, _ in p1.entries if not n.startswith("v_head.")] == [n for n, _, _ in p0.entries]
    assert p1.shape["v_head.w"] == (H,) and p1.shape["v_head.b"] == (1,) and p1.numel == p0.numel + H + 8
    w, b = p1.offset["v_head.w"], p1.offset["v_head.b"]
    assert w == p0.n_decay and p1.n_decay == w + H and p1.n_decay <= b < p1.n_opt and b + 8 == p1.n_opt      # placed as the reward head is
    assert p1.bucket_after["tail"] == (p0.bucket_after["tail"][0], p1.n_opt)
    assert len(list(p1.hf_names())) == len(list(p0.hf_names()))                          # not a checkpoint tensor
    l0, l1 = LoraLayout(cfg, 8), LoraLayout(dict(cfg, v_head=True), 8)
    assert {k: l1.offset[k] for k in l0.offset} == l0.offset and set(l1.offset) - set(l0.offset) == {"v_head.w", "v_head.b"}
    assert l1.offset["v_head.w"] == l0.numel and l1.n_decay == l0.numel + H == l1.offset["v_head.b"] and l1.numel == l1.n_decay + 8
    assert l1.hf_names() == l0.hf_names()
    with pytest.raises(ValueError, match="separate models"):
        ParamLayout(dict(cfg, v_head=True, rm_head=True))


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_ppo_exports_and_argument_errors_without_gpu():
    from vlrlhf import _hip
    l = _hip.lib()
    names = ("vlr_ppo_advantages", "vlr_ppo_loss", "vlr_v_head_bwd", "vlr_v_head_bwd_workspace_bytes")
    assert all(hasattr(l, n) and n in _hip.exported_symbols() for n in names)
    assert _hip.helper("vlr_abi_version") == 9                  # additive entry points: no caller breaks
    assert l.vlr_ppo_advantages(None, None, None, None, None, 0.2, 0, 1.0, 0.95, 0, None, None, None, None, 4, 2, None) == 1
    assert b"vlr_ppo_advantages" in l.vlr_last_error()
    assert l.vlr_ppo_loss(None, None, None, None, None, None, 4, 0.2, 0.2, 0.1, 10.0, 1.0, None, None, None, None) == 1
    assert b"vlr_ppo_loss" in l.vlr_last_error()
    assert l.vlr_v_head_bwd(None, None, None, None, None, None, 0, None, 4, 8, None) == 1 and b"vlr_v_head_bwd" in l.vlr_last_error()
    # shapes and modes are refused before anything is launched
    p = torch.zeros(64, dtype=torch.float32).data_ptr()
    for R, n in ((1, 1), (0, 1), (4, 0), (4, 5)):            # whitening needs two tokens; no sequences; more sequences than tokens
        assert l.vlr_ppo_advantages(p, p, p, p, p, 0.2, 0, 1.0, 0.95, 0, p, p, p, p, R, n, None) == 1
        assert b"vlr_ppo_advantages: bad shape" in l.vlr_last_error(), (R, n)
    for mode in (-1, 3):                                       # 3 would be "full"
        assert l.vlr_ppo_advantages(p, p, p, p, p, 0.2, mode, 1.0, 0.95, 0, p, p, p, p, 4, 2, None) == 1
        assert b"vlr_ppo_advantages: kl_penalty" in l.vlr_last_error()
    for R in (1, 0, -3):
        assert l.vlr_ppo_loss(p, p, p, p, p, p, R, 0.2, 0.2, 0.1, 10.0, 1.0, p, p, p, None) == 1 and b"vlr_ppo_loss: bad shape" in l.vlr_last_error()
    assert l.vlr_ppo_loss(p, p, p, p, p, p, 4, -0.1, 0.2, 0.1, 10.0, 1.0, p, p, p, None) == 1 and b"vlr_ppo_loss: negative" in l.vlr_last_error()
    for R, H in ((0, 8), (4, 4), (4, 12), (4, 0)):
        assert l.vlr_v_head_bwd(p, p, p, p, p, p, 0, p, R, H, None) == 1 and b"vlr_v_head_bwd: bad shape" in l.vlr_last_error(), (R, H)
    # the workspace: ceil(R / max(8, ceil(R / 256))) chunks of H + 1 floats
    for R, H in ((1, 8), (64, 136), (300, 4096), (32768, 4096)):
        rc = max(8, math.ceil(R / 256))
        assert l.vlr_v_head_bwd_workspace_bytes(R, H) == math.ceil(R / rc) * (H + 1) * 4
    assert l.vlr_v_head_bwd_workspace_bytes(0, 8) == 0


# ------------------------------------------------------------------------------------------------------------ the step's batch
def test_step_batch_layout_and_image_slicing():
    from types import SimpleNamespace
    from vlrlhf.base.trainer import VLPPOTrainer
    t = torch.tensor
    me = SimpleNamespace(padding_value=7)
    ids, mask, labels = VLPPOTrainer._build_batch(me, [t([1, 2, 3]), t([4])], [t([5]), t([6, 8, 9])])
    assert ids.tolist() == [[1, 2, 3, 5], [4, 6, 8, 9]] and mask.tolist() == [[1, 1, 1, 1]] * 2
    assert labels.tolist() == [[-100, -100, -100, 5], [-100, 6, 8, 9]]                   # every response token counts, nothing else
    ids, mask, labels = VLPPOTrainer._build_batch(me, [t([1]), t([4, 4])], [t([5]), t([6, 8])])
    assert ids.tolist() == [[1, 5, 7, 7], [4, 4, 6, 8]] and mask.tolist() == [[1, 1, 0, 0], [1, 1, 1, 1]] and labels[0].tolist() == [-100, 5, -100, -100]
    with pytest.raises(ValueError, match="empty"):
        VLPPOTrainer._build_batch(me, [t([1])], [t([], dtype=torch.long)])
    # rows carrying 2 and 1 images: tensors and per-image lists are cut by the counts, per-row lists by the rows, in minibatch order
    me = SimpleNamespace(model=SimpleNamespace(engine=SimpleNamespace(cfg=dict(image_token=9)), image_count_key="image_token"),
                         accelerator=SimpleNamespace(device="cpu"))
    ids = t([[9, 1, 9], [1, 9, 1]])
    img = dict(pixel_values=torch.arange(3.0).view(3, 1), names=["a0", "a1", "b0"], img_path=["a", "b"])
    out = VLPPOTrainer._rows_images(me, ids, img, [1, 0])
    assert out["pixel_values"].view(-1).tolist() == [2.0, 0.0, 1.0] and out["names"] == ["b0", "a0", "a1"] and out["img_path"] == ["b", "a"]
    assert VLPPOTrainer._rows_images(me, ids, {}, [0]) == {}
    with pytest.raises(ValueError, match="image input"):
        VLPPOTrainer._rows_images(me, ids, dict(pixel_values=torch.zeros(5, 1)), [0])
    with pytest.raises(ValueError, match="image input"):
        VLPPOTrainer._rows_images(me, ids, dict(pixel_values=torch.zeros(2, 1)), [0])      # a tensor is per image, never per row
    # 2, 0 and 1 images on three rows: three entries are one per row AND one per image, and the two readings differ - a list is refused,
    # a tensor is per image
    ids = t([[9, 1, 9], [1, 1, 1], [1, 9, 1]])
    with pytest.raises(ValueError, match="cannot be told apart"):
        VLPPOTrainer._rows_images(me, ids, dict(img_path=["a", "b", "c"]), [2, 0])
    out = VLPPOTrainer._rows_images(me, ids, dict(pixel_values=torch.arange(3.0)), [2, 1, 0])
    assert out["pixel_values"].tolist() == [2.0, 0.0, 1.0]
    # one image on every row: both readings agree
    ids = t([[9, 1], [1, 9]])
    assert VLPPOTrainer._rows_images(me, ids, dict(img_path=["a", "b"]), [1])["img_path"] == ["b"]


# ------------------------------------------------------------------------------------------------------------ collator, tokenize_row
def test_ppo_tokenize_row_and_collator_on_the_tiny_processor():
    from types import SimpleNamespace
    from tests.golden_util import TINY_PROCESSOR
    from vlrlhf.base.collator import VLPPODataCollator
    from vlrlhf.base.trainer import VLPPOTrainer
    from vlrlhf.models.Llava import LlavaPPODataCollator, LlavaProcessor
    proc = LlavaProcessor(TINY_PROCESSOR)
    proc.train()
    me = SimpleNamespace(processor=proc)
    img = torch.zeros(3, 28, 28)
    rows = [VLPPOTrainer.tokenize_row(me, dict(query="what is shown here?", img_path=img)),
            VLPPOTrainer.tokenize_row(me, dict(query="<image>\nand a longer question about the red car", image=img + 1))]
    for r in rows:
        assert set(r) == {"input_ids", "attention_mask", "query", "img_path"} and len(r["input_ids"]) == len(r["attention_mask"])      # no labels
        assert r["query"].count("<image>\n") == 1                          # the placeholder is added once, or kept
        # the ids are the single-turn conversation with an EMPTY answer: what the processor gives for it, ending where the assistant begins
        full = proc.process_batch_conv([proc.make_single_turn_conv(r["query"], "")])
        assert r["input_ids"] == full["full"]["input_ids"][0] and full["raw_str"][0].endswith(proc.chat_template.assistant_begin)
        assert r["input_ids"].count(proc.tokenizer.convert_tokens_to_ids("<image>")) == 1
    assert torch.equal(rows[1]["img_path"], img + 1)                       # the reference's `image` key is read too
    assert VLPPOTrainer._tokenize_dataset(me, rows) == rows and VLPPOTrainer._tokenize_dataset(me, None) is None      # tokenised rows pass through
    # the base collator: lists, nothing padded; ids and mask as one LongTensor per row
    batch = VLPPODataCollator()(rows)
    assert set(batch) == set(rows[0]) and all(isinstance(v, list) and len(v) == 2 for v in batch.values())
    assert [t.tolist() for t in batch["input_ids"]] == [r["input_ids"] for r in rows] and batch["input_ids"][0].dtype == torch.long
    assert batch["attention_mask"][1].dtype == torch.long and batch["query"] == [r["query"] for r in rows]
    assert len(batch["input_ids"][0]) != len(batch["input_ids"][1])
    # the LLaVA collator adds the rows' images
    batch = LlavaPPODataCollator(proc)(rows)
    assert batch["pixel_values"].shape == (2, 3, 28, 28) and torch.equal(batch["pixel_values"][1], img + 1)
    # the trainer's batches: shuffled, whole batches only
    me = SimpleNamespace(dataset=[dict(r, n=i) for i, r in enumerate(rows * 3)][:5], config=SimpleNamespace(batch_size=2),
                         data_collator=VLPPODataCollator(), _data_gen=torch.Generator().manual_seed(4))
    seen = [b["n"] for b in VLPPOTrainer.get_batches(me)]
    assert len(seen) == 2 and all(len(b) == 2 for b in seen) and len({i for b in seen for i in b}) == 4


# ------------------------------------------------------------------------------------------------------------ vlrlhf/ppo.py
def test_ppo_script_arguments_rules_and_refusals(tmp_path, capsys):
    import json
    from vlrlhf import ppo
    # --help lists the reference's arguments
    with pytest.raises(SystemExit):
        ppo._parse(["--help"])
    out = capsys.readouterr().out
    for name in ("data_dir", "image_root", "model_name_or_path", "reward_adapter", "reward_adapter_name", "reward_model_name_or_path",
                 "ignore_bias_buffers", "freeze_vision_tower", "v_head_init_strategy", "v_head_initializer_range", "lora_r", "lora_alpha",
                 "lora_dropout", "lora_target_modules", "lora_bias", "q_lora", "bits", "modules_to_save", "use_lora", "use_value_adapter",
                 "run_name", "project_name", "group_name", "gradient_checkpointing", "fp16", "bf16", "tf32", "fsdp", "local_rank", "output_dir",
                 "per_device_gamelog_size", "max_new_tokens", "max_length", "learning_rate", "batch_size", "mini_batch_size",
                 "gradient_accumulation_steps", "ppo_epochs", "gamma", "lam", "cliprange", "cliprange_value", "vf_coef", "kl_penalty",
                 "init_kl_coef", "adap_kl_ctrl", "target", "horizon", "whiten_rewards", "ratio_threshold", "early_stopping", "target_kl",
                 "max_grad_norm", "seed"):
        assert f"--{name} " in out or f"--{name}\n" in out, name
    sa, cfg, la = ppo._parse(["--batch_size", "4", "--mini_batch_size", "2", "--max_new_tokens", "16", "--use_lora", "true", "--whiten_rewards", "True",
                              "--max_grad_norm", "1.0", "--report_to", "wandb"])
    assert "[vlrlhf.ppo] WARNING: ignoring unsupported arguments: --report_to wandb" in capsys.readouterr().err
    assert (cfg.batch_size, cfg.mini_batch_size, cfg.max_new_tokens, cfg.max_length, cfg.use_lora, cfg.whiten_rewards, cfg.max_grad_norm) == \
        (4, 2, 16, None, True, True, 1.0)
    assert sa.v_head_init_strategy == "normal" and sa.v_head_initializer_range == 0.2 and sa.freeze_vision_tower and la.lora_r == 64
    # the argument rules of the reference's PPOConfig
    with pytest.raises(ValueError, match="per_device_gamelog_size should be less than batch_size"):
        ppo.PPOConfig(batch_size=2, mini_batch_size=2, per_device_gamelog_size=3)
    ppo.PPOConfig(batch_size=2, mini_batch_size=2, per_device_gamelog_size=2)
    with pytest.raises(ValueError, match="only use one of max_new_tokens and max_length"):
        ppo.PPOConfig(batch_size=2, mini_batch_size=2, max_new_tokens=8, max_length=64)
    with pytest.raises(ValueError, match="one of fp16 and bf16"):
        ppo.PPOConfig(batch_size=2, mini_batch_size=2, fp16=True, bf16=True)
    with pytest.raises(ValueError, match="value adapter with a Peft base model"):
        ppo.PPOConfig(batch_size=2, mini_batch_size=2, use_value_adapter=True)
    # refusals of main(), before anything is loaded
    base = ["--batch_size", "2", "--mini_batch_size", "2", "--model_name_or_path", str(tmp_path)]
    with pytest.raises(NotImplementedError, match="freeze_vision_tower False"):
        ppo.main(base + ["--freeze_vision_tower", "False", "--reward_model_name_or_path", "x"])
    with pytest.raises(ValueError, match="only use one of reward_adapter and reward_model"):
        ppo.main(base + ["--reward_adapter", "a", "--reward_model_name_or_path", "x"])
    with pytest.raises(NotImplementedError, match="reward_adapter"):
        ppo.main(base + ["--reward_adapter", "a"])
    with pytest.raises(NotImplementedError, match="use_value_adapter"):
        ppo.main(base + ["--use_value_adapter", "true", "--use_lora", "true", "--reward_model_name_or_path", "x"])
    with pytest.raises(ValueError, match="needs a reward model"):
        ppo.main(base)
    with pytest.raises(NotImplementedError, match="q_lora"):
        ppo.lora_config_from_args(None, ppo.PPOConfig(batch_size=2, mini_batch_size=2, use_lora=True), ppo.LoraArguments(q_lora=True))
    assert ppo.lora_config_from_args(None, ppo.PPOConfig(batch_size=2, mini_batch_size=2), ppo.LoraArguments()) is None
    # the generation config: top_p = 1.0, and the length limit the PPO config names
    for arch, stops in (("LlavaForConditionalGeneration", None), ("QWenLMHeadModel", [[151645], [151644]])):
        with open(tmp_path / "config.json", "w") as f:
            json.dump(dict(architectures=[arch]), f)
        with open(tmp_path / "generation_config.json", "w") as f:
            json.dump(dict(top_p=0.3, top_k=0, eos_token_id=2, max_new_tokens=512, transformers_version="4.41.0"), f)
        gc = ppo.generation_config_for(str(tmp_path), ppo.PPOConfig(batch_size=2, mini_batch_size=2, max_new_tokens=16))
        assert gc.top_p == 1.0 and gc.max_new_tokens == 16 and gc.eos_token_id == 2 and getattr(gc, "stop_words_ids", None) == stops
        gc = ppo.generation_config_for(str(tmp_path), ppo.PPOConfig(batch_size=2, mini_batch_size=2, max_length=64))
        assert gc.top_p == 1.0 and gc.max_length == 64 and gc.max_new_tokens is None
    for arch in ("LlavaNextForConditionalGeneration", "InternLMXComposer2ForCausalLM"):
        with open(tmp_path / "config.json", "w") as f:
            json.dump(dict(architectures=[arch]), f)
        from vlrlhf.utils.auto_load import MyAutoModelWithValueHead, MyAutoPPOCollator
        with pytest.raises(NotImplementedError, match="LLaVA-1.5 and Qwen-VL"):
            MyAutoModelWithValueHead.from_pretrained(str(tmp_path))
        with pytest.raises(NotImplementedError, match="LLaVA-1.5 and Qwen-VL"):
            MyAutoPPOCollator(str(tmp_path))
    rows = ppo.make_synthetic_query_dataset(ppo.ScriptArguments(synthetic_rows=3, synthetic_image_size=28))
    assert len(rows) == 3 and set(rows[0]) == {"query", "image", "img_path"} and rows[0]["img_path"].shape == (3, 28, 28)
