"""GRPO without a GPU: the checker's own arithmetic (tests/grpo_ref.py) on hand-computed cases, the argument rules of GRPOConfig, the
refusals of VLGRPOTrainer and vlrlhf/grpo.py, the GRPO registry beside the untouched PPO one, the exports and argument errors of the two
new entry points, and the rows of a group (queries and image inputs expanded in repeat_interleave order)."""
import math
import os

import pytest
import torch

from tests import grpo_ref as GR

LN2 = math.log(2.0)


# ------------------------------------------------------------------------------------------------------------ the checker, by hand
def test_advantages_by_hand_2x3():
    s = torch.tensor([1.0, 2.0, 3.0, 2.0, 2.0, 2.0]).double()
    A, st = GR.advantages(s, 2, 3, True)                      # group 0: mean 2, unbiased std 1; group 1: all equal
    assert torch.allclose(A, torch.tensor([-1.0, 0.0, 1.0, 0.0, 0.0, 0.0]).double() / (1.0 + 1e-4), rtol=0, atol=1e-15)
    assert A[3:].tolist() == [0.0, 0.0, 0.0]                  # exactly 0, never NaN
    assert st.tolist() == [2.0, 0.5, 0.5]
    A, st = GR.advantages(s, 2, 3, False)
    assert A.tolist() == [-1.0, 0.0, 1.0, 0.0, 0.0, 0.0] and st.tolist() == [2.0, 0.5, 0.5]
    # the unbiased form: [0, 2] has std sqrt(2), the biased one would be 1
    A, st = GR.advantages(torch.tensor([0.0, 2.0]).double(), 1, 2, True)
    assert abs(float(st[1]) - math.sqrt(2.0)) < 1e-15 and abs(float(A[1]) - 1.0 / (math.sqrt(2.0) + 1e-4)) < 1e-15
    # equal fp32 scores that no fp32 mean reproduces: the fp64 replay still has std == 0
    A, st = GR.advantages(torch.tensor([0.1, 0.1, 0.1]).double(), 1, 3, True)
    assert A.tolist() == [0.0, 0.0, 0.0] and float(st[2]) == 1.0


def _hand_case():
    """2 sequences, 5 tokens.  Sequence 0 (A = 1): ratio 1 (inside), ratio 2 (clipped high).  Sequence 1 (A = -2): ratio 1 (inside),
    ratio 0.5 (clipped low), ratio 2 (outside the range, the unclipped branch is the smaller one)"""
    old = torch.tensor([-1.0, -2.0, -1.5, -1.0, -3.0]).double()
    logp = old + torch.tensor([0.0, LN2, 0.0, -LN2, LN2], dtype=torch.float64)
    return logp, old, torch.tensor([1.0, -2.0]).double(), [0, 2, 5]


@pytest.mark.parametrize("loss_type,want,weights", [
    ("grpo", 0.5 * ((-1.0 - 1.2) / 2 + (2.0 + 1.6 + 4.0) / 3), [1 / 4, 1 / 4, 1 / 6, 1 / 6, 1 / 6]),
    ("bnpo", (-2.2 + 7.6) / 5, [1 / 5] * 5),
    ("dr_grpo", (-2.2 + 7.6) / (2 * 4), [1 / 8] * 5),
])
def test_loss_by_hand_2_sequences_5_tokens(loss_type, want, weights):
    logp, old, adv, so = _hand_case()
    st, dlogp = GR.loss_and_grad(logp, old, None, adv, so, 0.2, 0.2, 0.0, loss_type, 4)
    assert abs(st["loss"] - want) < 1e-12
    # d l / d logp: -A r inside (tie halved, both halves equal) = -1, 2; 0 on the clipped side; -A r = 4 outside on the unclipped branch
    exp = torch.tensor([-1.0, 0.0, 2.0, 0.0, 4.0]).double() * torch.tensor(weights, dtype=torch.float64)
    assert torch.allclose(dlogp, exp, rtol=0, atol=1e-12) and dlogp[1] == 0 and dlogp[3] == 0
    assert st["clip_low"] == 0.2 and st["clip_high"] == 0.2 and abs(st["clip_region"] - 0.4) < 1e-15
    assert abs(st["ratio"] - 1.3) < 1e-12 and st["len_mean"] == 2.5 and st["kl"] == 0.0
    assert GR.branch_counts(logp, old, adv, so, 0.2, 0.2) == dict(inside=2, clipped_low=1, clipped_high=1, outside_unclipped=1, zero_advantage=0)
    # upstream scales the gradient, not the reported loss
    st2, d2 = GR.loss_and_grad(logp, old, None, adv, so, 0.2, 0.2, 0.0, loss_type, 4, upstream=0.25)
    assert st2["loss"] == st["loss"] and torch.allclose(d2, 0.25 * dlogp, rtol=0, atol=1e-15)


def test_loss_by_hand_kl_null_old_and_zero_eps():
    logp, old, adv, so = _hand_case()
    # the KL term on one token: d = ln 2 -> k = 2 - ln 2 - 1, d k / d logp = 1 - 2 = -1
    ref = logp + torch.tensor([0.0, 0.0, LN2, 0.0, 0.0], dtype=torch.float64)
    st0, g0 = GR.loss_and_grad(logp, old, None, adv, so, 0.2, 0.2, 0.0, "bnpo")
    st, g = GR.loss_and_grad(logp, old, ref, adv, so, 0.2, 0.2, 0.5, "bnpo")
    k = 1.0 - LN2
    assert abs(st["kl"] - k / 5) < 1e-12 and abs(st["loss"] - (st0["loss"] + 0.5 * k / 5)) < 1e-12
    assert torch.allclose(g - g0, torch.tensor([0.0, 0.0, -0.5 / 5, 0.0, 0.0], dtype=torch.float64), rtol=0, atol=1e-12)
    # old_logp None: the ratio is exactly 1 everywhere, nothing is clipped, the gradient is -A w; and equals old_logp = a copy of logp
    st, g = GR.loss_and_grad(logp, None, None, adv, so, 0.2, 0.2, 0.0, "bnpo")
    st_c, g_c = GR.loss_and_grad(logp, logp.clone(), None, adv, so, 0.2, 0.2, 0.0, "bnpo")
    assert st["ratio"] == 1.0 and st["clip_region"] == 0.0 and g.tolist() == [-0.2, -0.2, 0.4, 0.4, 0.4] and torch.equal(g, g_c) and st == st_c
    assert abs(st["loss"] - (-2.0 + 6.0) / 5) < 1e-15
    # eps = 0: the ratio sits ON both bounds - the closed interval passes the gradient, the tie halves two equal halves: still -A w
    st, g = GR.loss_and_grad(logp, None, None, adv, so, 0.0, 0.0, 0.0, "bnpo")
    assert g.tolist() == [-0.2, -0.2, 0.4, 0.4, 0.4] and st["clip_region"] == 0.0
    # an advantage of 0: no policy gradient at all
    st, g = GR.loss_and_grad(logp, old, None, torch.tensor([0.0, -2.0]).double(), so, 0.2, 0.2, 0.0, "grpo")
    assert g[:2].tolist() == [0.0, 0.0] and GR.branch_counts(logp, old, torch.tensor([0.0, -2.0]), so, 0.2, 0.2)["zero_advantage"] == 2


# ------------------------------------------------------------------------------------------------------------ config, refusals, registry
def test_grpo_config_defaults_and_rules():
    from vlrlhf.base.trainer import GRPOConfig
    c = GRPOConfig()
    assert (c.num_generations, c.num_iterations, c.beta, c.epsilon, c.epsilon_high, c.loss_type, c.scale_rewards) == (8, 1, 0.04, 0.2, None, "grpo", True)
    c = GRPOConfig(batch_size=2, num_generations=4, mini_batch_size=2, gradient_accumulation_steps=2)
    assert c.rows == 8 and c.backward_batch_size == 4
    for bad in (dict(batch_size=2, num_generations=3, mini_batch_size=4), dict(batch_size=2, num_generations=4, mini_batch_size=4, gradient_accumulation_steps=3),
                dict(batch_size=1, num_generations=2, mini_batch_size=0)):
        with pytest.raises(ValueError, match="multiple"):
            GRPOConfig(**bad)
    with pytest.raises(ValueError, match="num_generations"):
        GRPOConfig(batch_size=2, num_generations=1, mini_batch_size=2)
    with pytest.raises(ValueError, match="batch_size"):
        GRPOConfig(batch_size=0, num_generations=2, mini_batch_size=2)
    with pytest.raises(ValueError, match="num_iterations"):
        GRPOConfig(batch_size=1, num_generations=2, mini_batch_size=2, num_iterations=0)
    with pytest.raises(ValueError, match="beta"):
        GRPOConfig(batch_size=1, num_generations=2, mini_batch_size=2, beta=-0.1)
    with pytest.raises(ValueError, match="epsilon"):
        GRPOConfig(batch_size=1, num_generations=2, mini_batch_size=2, epsilon_high=-0.1)
    with pytest.raises(ValueError, match="loss_type"):
        GRPOConfig(batch_size=1, num_generations=2, mini_batch_size=2, loss_type="dapo")
    with pytest.raises(ValueError, match="max_new_tokens"):
        GRPOConfig(batch_size=1, num_generations=2, mini_batch_size=2, loss_type="dr_grpo")
    GRPOConfig(batch_size=1, num_generations=2, mini_batch_size=2, loss_type="dr_grpo", max_new_tokens=8)


def test_grpo_trainer_refusals_before_anything_is_built():
    from types import SimpleNamespace
    from vlrlhf.base.trainer import GRPOConfig, VLGRPOTrainer
    cfg = GRPOConfig(batch_size=1, num_generations=2, mini_batch_size=2)
    with pytest.raises(ValueError, match="config and a model"):
        VLGRPOTrainer(cfg, None)
    with pytest.raises(ValueError, match="no value head"):
        VLGRPOTrainer(cfg, SimpleNamespace(v_head=object()))
    with pytest.raises(NotImplementedError, match="more than one GPU has never been run"):
        VLGRPOTrainer(GRPOConfig(batch_size=1, num_generations=2, mini_batch_size=2, world_size=2), SimpleNamespace())
    with pytest.raises(ValueError, match="one of reward_model and reward_fn"):
        VLGRPOTrainer(cfg, SimpleNamespace(), reward_model=object(), reward_fn=lambda q, r: [])
    me = SimpleNamespace(reward_fn=None, reward_model=None)
    with pytest.raises(NotImplementedError, match="reward source"):
        VLGRPOTrainer.score(me, ["q"], ["r"], {})
    with pytest.raises(NotImplementedError, match="reward source"):
        VLGRPOTrainer.train(me)
    me = SimpleNamespace(reward_fn=lambda q, r: [1.0], reward_model=None)
    with pytest.raises(ValueError, match="returned 1 scores for 2"):
        VLGRPOTrainer.score(me, ["q", "q"], ["a", "b"], {})
    me = SimpleNamespace(reward_fn=lambda q, r: [len(x) for x in r], reward_model=None)
    assert VLGRPOTrainer.score(me, ["q", "q"], ["a", "bcd"], {}) == [1.0, 3.0]


def test_grpo_registry_beside_the_untouched_ppo_one():
    from vlrlhf.base.trainer import VLGRPOTrainer, VLOnlineRLTrainer, VLPPOTrainer
    from vlrlhf.models import InternLMXC2, Llava, LlavaNext, QwenVL
    from vlrlhf.utils import auto_load
    assert auto_load.GRPO_FAMILIES == ["Llava", "QwenVL"] and auto_load.PPO_FAMILIES == ["Llava", "QwenVL"] and auto_load.RM_FAMILIES == ["Llava", "QwenVL"]
    for arch, pkg in (("LlavaForConditionalGeneration", Llava), ("QWenLMHeadModel", QwenVL)):
        tr = auto_load._grpo_slot(arch, "trainer")
        assert tr is pkg.grpo_core.trainer and issubclass(tr, VLGRPOTrainer) and issubclass(tr, VLOnlineRLTrainer) and not issubclass(tr, VLPPOTrainer)
        assert pkg.grpo_core.model is pkg.core_mapper.model and pkg.grpo_core.collator is pkg.ppo_core.collator
        assert pkg.core_mapper.model.image_count_key == pkg.ppo_core.value_model.image_count_key
    for arch in ("LlavaNextForConditionalGeneration", "InternLMXComposer2ForCausalLM"):
        with pytest.raises(NotImplementedError, match="LLaVA-1.5 and Qwen-VL"):
            auto_load._grpo_slot(arch, "trainer")
    assert not hasattr(LlavaNext, "grpo_core") and not hasattr(InternLMXC2, "grpo_core")
    # the shared methods are the base's: PPO's behaviour is the code it had
    for name in ("tokenize_row", "get_batches", "compute_scores", "_build_batch", "_rows_images", "_generate_rows", "save_checkpoint", "load_checkpoint"):
        assert getattr(VLPPOTrainer, name) is getattr(VLOnlineRLTrainer, name) is getattr(VLGRPOTrainer, name), name
    assert VLPPOTrainer.generate is VLOnlineRLTrainer.generate and VLGRPOTrainer.generate is not VLOnlineRLTrainer.generate


# ------------------------------------------------------------------------------------------------------------ the rows of a group
def test_group_rows_queries_and_images_expand_in_repeat_interleave_order():
    from types import SimpleNamespace
    from vlrlhf.base.trainer import GRPOConfig, VLGRPOTrainer
    t = torch.tensor
    me = SimpleNamespace(config=GRPOConfig(batch_size=2, num_generations=3, mini_batch_size=3),
                         model=SimpleNamespace(engine=SimpleNamespace(cfg=dict(image_token=9)), image_count_key="image_token"),
                         accelerator=SimpleNamespace(device="cpu"))
    me._rows_images = lambda ids, img, rows: VLGRPOTrainer._rows_images(me, ids, img, rows)
    qs = [t([9, 1, 9]), t([1, 9])]                            # 2 images, 1 image
    assert [q.tolist() for q in VLGRPOTrainer._expand_queries(me, qs)] == [[9, 1, 9]] * 3 + [[1, 9]] * 3
    out = VLGRPOTrainer._expand_images(me, qs, dict(pixel_values=torch.arange(3.0).view(3, 1), img_path=["a", "b"]))
    assert out["pixel_values"].view(-1).tolist() == [0.0, 1.0] * 3 + [2.0] * 3 and out["img_path"] == ["a"] * 3 + ["b"] * 3
    assert VLGRPOTrainer._expand_images(me, qs, {}) == {}
    # responses that ran to the limit without a stop
    me = SimpleNamespace(config=SimpleNamespace(max_new_tokens=3), generation_kwargs=dict(eos_token_id=2), model=None,
                         _stop_rules=lambda model, kw: ({2}, [[5, 6]]))
    rs = [t([1, 1, 1]), t([1, 1, 2]), t([1, 5, 6]), t([1, 1])]  # cut; ended by eos at the limit; ended by a stop word; short
    assert VLGRPOTrainer._clipped_frac(me, rs) == 0.25


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_grpo_exports_header_and_argument_errors_without_gpu():
    from vlrlhf import _hip
    l = _hip.lib()
    names = ("vlr_grpo_advantages", "vlr_grpo_loss")
    assert all(hasattr(l, n) and n in _hip.exported_symbols() for n in names)
    assert _hip.helper("vlr_abi_version") == 9                  # additive entry points: no caller breaks
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "vlr.h")) as f:
        header = f.read()
    assert "---- GRPO" in header and all(f"int {n}(" in header for n in names)
    with open(os.path.join(root, "vl-rlhf_amd", "build_hip.py")) as f:
        assert '"grpo.hip"' in f.read()
    p = torch.zeros(64, dtype=torch.float32).data_ptr()
    adv = lambda *a: l.vlr_grpo_advantages(*a, None)           # noqa: E731
    assert adv(None, 2, 2, 1, p, p) == 1 and b"vlr_grpo_advantages: null operand" in l.vlr_last_error()
    assert adv(p, 2, 2, 1, None, p) == 1 and adv(p, 2, 2, 1, p, None) == 1
    for P, G in ((0, 2), (1, 1), (1, 0), (-1, 4)):            # no prompt; the unbiased std needs two samples
        assert adv(p, P, G, 1, p, p) == 1 and l.vlr_last_error().startswith(b"vlr_grpo_advantages: bad shape"), (P, G)
    loss = lambda *a: l.vlr_grpo_loss(*a, None)               # noqa: E731
    ok = dict(logp=p, old=p, ref=p, adv=p, so=p, R=4, n=2, el=0.2, eh=0.2, beta=0.04, lt=0, mcl=0, up=1.0, d=p, st=p)
    call = lambda **kw: loss(*{**ok, **kw}.values())          # noqa: E731
    for k in ("logp", "adv", "so", "d", "st"):
        assert call(**{k: None}) == 1 and l.vlr_last_error().startswith(b"vlr_grpo_loss: null operand"), k
    assert call(ref=None) == 1 and l.vlr_last_error().startswith(b"vlr_grpo_loss: null ref_logp")      # beta != 0 needs the reference
    for R, n in ((0, 1), (4, 0), (4, 5), (-2, 1)):
        assert call(R=R, n=n) == 1 and l.vlr_last_error().startswith(b"vlr_grpo_loss: bad shape"), (R, n)
    for kw in (dict(el=-0.1), dict(eh=-1e-9)):
        assert call(**kw) == 1 and l.vlr_last_error().startswith(b"vlr_grpo_loss: negative clip range")
    for lt in (-1, 3):
        assert call(lt=lt) == 1 and l.vlr_last_error().startswith(b"vlr_grpo_loss: loss_type")
    assert call(lt=2, mcl=0) == 1 and l.vlr_last_error().startswith(b"vlr_grpo_loss: max_completion_length")


# ------------------------------------------------------------------------------------------------------------ vlrlhf/grpo.py
def test_grpo_script_arguments_and_refusals(tmp_path, capsys):
    import json
    from vlrlhf import grpo
    with pytest.raises(SystemExit):
        grpo._parse(["--help"])
    out = capsys.readouterr().out
    for name in ("data_dir", "image_root", "model_name_or_path", "reward_model_name_or_path", "freeze_vision_tower", "dataset_name", "synthetic_rows",
                 "lora_r", "lora_alpha", "lora_dropout", "lora_target_modules", "q_lora", "use_lora", "batch_size", "num_generations",
                 "mini_batch_size", "gradient_accumulation_steps", "num_iterations", "beta", "epsilon", "epsilon_high", "loss_type",
                 "scale_rewards", "max_new_tokens", "learning_rate", "max_grad_norm", "seed", "save_steps", "output_dir", "gradient_checkpointing",
                 "run_name", "project_name", "group_name", "fp16", "bf16", "tf32", "fsdp", "resume_from_checkpoint"):
        assert f"--{name} " in out or f"--{name}\n" in out, name
    sa, cfg, la = grpo._parse(["--batch_size", "2", "--num_generations", "4", "--mini_batch_size", "4", "--max_new_tokens", "16", "--use_lora", "true",
                               "--loss_type", "dr_grpo", "--beta", "0", "--epsilon_high", "0.28", "--scale_rewards", "False", "--report_to", "wandb"])
    assert "[vlrlhf.grpo] WARNING: ignoring unsupported arguments: --report_to wandb" in capsys.readouterr().err
    assert (cfg.batch_size, cfg.num_generations, cfg.mini_batch_size, cfg.max_new_tokens, cfg.use_lora, cfg.loss_type, cfg.beta, cfg.epsilon_high,
            cfg.scale_rewards) == (2, 4, 4, 16, True, "dr_grpo", 0.0, 0.28, False)
    assert sa.freeze_vision_tower and la.lora_r == 64 and cfg.rows == 8
    with pytest.raises(ValueError, match="one of fp16 and bf16"):
        grpo.GRPOConfig(batch_size=1, num_generations=2, mini_batch_size=2, fp16=True, bf16=True)
    # refusals of main(), before anything is loaded
    base = ["--batch_size", "1", "--num_generations", "2", "--mini_batch_size", "2", "--model_name_or_path", str(tmp_path)]
    fn = lambda q, r: [0.0] * len(r)                           # noqa: E731
    with pytest.raises(NotImplementedError, match="freeze_vision_tower False"):
        grpo.main(base + ["--freeze_vision_tower", "False"], reward_fn=fn)
    with pytest.raises(NotImplementedError, match="q_lora"):
        grpo.main(base + ["--use_lora", "true", "--q_lora", "true"], reward_fn=fn)
    with pytest.raises(NotImplementedError, match="more than one GPU has never been run"):
        grpo.main(base + ["--world_size", "2"], reward_fn=fn)
    with pytest.raises(ValueError, match="needs a reward source"):
        grpo.main(base)
    with pytest.raises(ValueError, match="only use one of"):
        grpo.main(base + ["--reward_model_name_or_path", "x"], reward_fn=fn)
    for arch in ("LlavaNextForConditionalGeneration", "InternLMXComposer2ForCausalLM"):
        with open(tmp_path / "config.json", "w") as f:
            json.dump(dict(architectures=[arch]), f)
        with pytest.raises(NotImplementedError, match="LLaVA-1.5 and Qwen-VL"):
            grpo.main(base, reward_fn=fn)
        from vlrlhf.utils.auto_load import MyAutoGRPOCollator, MyAutoGRPOTrainer
        with pytest.raises(NotImplementedError, match="LLaVA-1.5 and Qwen-VL"):
            MyAutoGRPOTrainer(str(tmp_path))
        with pytest.raises(NotImplementedError, match="LLaVA-1.5 and Qwen-VL"):
            MyAutoGRPOCollator(str(tmp_path))
    with pytest.raises(NotImplementedError, match="q_lora"):
        grpo.lora_config_from_args(None, grpo.GRPOConfig(batch_size=1, num_generations=2, mini_batch_size=2, use_lora=True), grpo.LoraArguments(q_lora=True))
    assert grpo.lora_config_from_args(None, grpo.GRPOConfig(batch_size=1, num_generations=2, mini_batch_size=2), grpo.LoraArguments()) is None
    rows = grpo.make_synthetic_query_dataset(grpo.ScriptArguments(synthetic_rows=3, synthetic_image_size=28))
    assert len(rows) == 3 and set(rows[0]) == {"query", "image", "img_path"}
