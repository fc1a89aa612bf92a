"""Reward-model training and scoring on the MI355X (LLaVA-1.5 and Qwen-VL) against the CPU oracles run on EACH HALF ALONE (tests/rm_ref.py):
the ONE concatenated pass reads every sequence's reward at the last column of its own half - a padding row for the shorter sequences of
both fixtures - and must give the rewards, the pair loss and the gradients of the reference's two passes.  Also: the lm-head's zero
gradient (the reference's 0.0 * mean(logits) line), weight decay on it, LoRA with the head trained beside the adapters, score(), the
save / load round trip, eval accuracy with ties, and an eight-step trajectory.  Needs a real MI355X:  pytest -m gpu"""
import functools
import os
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import llava_dpo_oracle as O  # noqa: E402  (checker only)
from tests import rm_ref as R  # noqa: E402
from tests.golden_util import load_case  # noqa: E402
from tests.test_hip_e2e import EMU, PEFT, cosine, gpu, relmax  # noqa: E402,F401

CASES = ("llava_hipsmall", "qwenvl_small")
# max |HIP - fp32 oracle of each half alone|, measured on an MI355X (profiles/reward_model.txt) and doubled: the factor covers run-to-run
# kernel selection and a later compiler.  Measured: rewards 6.851e-3 (LLaVA) / 1.991e-2 (Qwen-VL), loss 1.163e-3 / 1.970e-3.
# For scale: the oracle's own bf16 emulation of the decoder (O.HIP_ROUNDING) sits 5.0e-3 (LLaVA) / 6.5e-3 (Qwen-VL) from its fp32 rewards on
# these fixtures.  LLaVA is of that order.  Qwen-VL is three times it, on ONE reward (rejected[0]: -0.2719 against -0.2520; the other three
# are within 6.1e-3), and the cause is the vision tower: the HIP path runs Qwen-VL's whole tower and resampler in bf16, which O.HIP_ROUNDING
# does not model.  Rounding the tower alone in the oracle (emulate_bf16={"vit"}, part of tests/test_hip_qwenvl.py's set) moves its rewards
# by up to 2.9e-2 and this one by -1.9e-2, where the HIP value sits (-2.0e-2); the emulation does not reproduce the tower's roundings op
# for op, so the other rewards do not follow it.  Both distances are recorded next to the fp32 figures.
TOL_REWARD = {"llava_hipsmall": 1.37e-2, "qwenvl_small": 3.98e-2}
TOL_LOSS = {"llava_hipsmall": 2.33e-3, "qwenvl_small": 3.94e-3}
TOL_TRAJECTORY = 4.99e-3      # per-step |HIP loss - oracle-loop loss| over the eight steps (measured 2.495e-3), doubled the same way
GRAD_COS, GRAD_RELMAX = 0.995, 8e-2      # the bounds of tests/test_hip_sft.py on one step's gradients against oracle autograd
DEFAULT_OPTIM = dict(lr=1e-3, beta1=0.9, beta2=0.98, eps=1e-6, weight_decay=0.05, max_grad_norm=1.0)


def _optim(cfg):
    return dict(cfg.get("optim") or DEFAULT_OPTIM)


def build(case, lora=None, head=None):
    from vlrlhf.models.Llava import LlavaRewardModel, LlavaRMTrainer
    from vlrlhf.models.QwenVL import QwenVLRewardModel, QwenVLRMTrainer
    z, cfg, W, W_ref, batch, _ = load_case(case)
    qwen = "visual" in cfg
    model = (QwenVLRewardModel if qwen else LlavaRewardModel).from_state_dict(cfg, W, rm_head=head or R.rm_head(cfg["hidden"]))
    o = _optim(cfg)
    args = SimpleNamespace(gradient_accumulation_steps=1, per_device_train_batch_size=2, learning_rate=o["lr"], adam_beta1=o["beta1"],
                           adam_beta2=o["beta2"], adam_epsilon=o["eps"], weight_decay=o["weight_decay"], max_grad_norm=o["max_grad_norm"], seed=0)
    tr = (QwenVLRMTrainer if qwen else LlavaRMTrainer)(model, args, None, None, None, None, peft_config=lora)
    return cfg, W, R.rm_batch(batch), model, tr


# names of the tensors whose gradients are compared: the head, the last and the first decoder layer's q|k|v and down projections, the embedding
def _grad_names(cfg):
    L = cfg["layers"]
    if "visual" in cfg:
        per = lambda l: [f"transformer.h.{l}.attn.c_attn.weight", f"transformer.h.{l}.mlp.c_proj.weight"]      # noqa: E731
        return per(L - 1) + per(0) + ["transformer.wte.weight"], "lm_head.weight"
    p = "language_model.model.layers."
    per = lambda l: [f"{p}{l}.self_attn.{n}_proj.weight" for n in "qkv"] + [f"{p}{l}.mlp.down_proj.weight"]      # noqa: E731
    return per(L - 1) + per(0) + ["language_model.model.embed_tokens.weight"], "language_model.lm_head.weight"


@functools.lru_cache(maxsize=None)
def oracle(case):
    """fp32 oracle of each half alone, computed once per fixture and shared: (loss, r_chosen, r_rejected, gradients, per-half aux)"""
    z, cfg, W, W_ref, batch, _ = load_case(case)
    w, b = R.rm_head(cfg["hidden"])
    names = [n for n in O.trainable_names(W) if not n.startswith("transformer.visual.")]
    return R.loss_and_grads(W, cfg, R.rm_batch(batch), w, b, names)


def _record(line):
    f = os.environ.get("VLR_RM_MARGINS")
    print(line)
    if f:
        with open(f, "a") as fh:
            fh.write(line + "\n")


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("case", CASES)
def test_rewards_loss_and_gradients_match_oracle_of_each_half_alone(gpu, case):
    cfg, W, rb, model, tr = build(case)
    exp_loss, exp_c, exp_r, exp_g = oracle(case)
    eng = model.engine
    eng.init_optimizer()
    model.train()
    loss, out = tr.compute_loss(model, tr._prepare_inputs(rb), return_outputs=True)
    rc, rr = out["rewards_chosen"], out["rewards_rejected"]
    assert rc.dtype == torch.float32 and rc.shape == (2,) and loss.dtype == torch.float32
    # ---- the masked rows the rewards are read at: embedding and position as the oracle's merge leaves them
    c = model.base_model._last_ctx
    Bn, S, T, H = c["Bn"], c["S"], c["T"], eng.H
    x0, pos, img = c["x0"].view(Bn, S, H).float().cpu(), c["pos"].view(Bn, S).cpu(), c["img_map"].view(Bn, S).cpu()
    px = rb["img_input_dict"]["pixel_values"]
    for h, side in enumerate(("chosen", "rejected")):
        ids, mask = rb[f"input_ids_{side}"], rb[f"attention_mask_{side}"]
        if "visual" in cfg:
            from oracle import qwenvl_oracle as Q
            aux = Q.qwenvl_forward(W, cfg, ids, mask, px.float(), return_hidden=True, dedupe_images=False)[2]
            o_pos = torch.arange(ids.shape[1])[None].expand(2, -1)
        else:
            aux = O.llava_forward(W, cfg, ids, mask, None, px.float(), dedupe_images=False, return_hidden=True)[2]
            o_pos = aux["pos"]
        Sh = aux["merged"].shape[1]
        assert Sh == ids.shape[1] + (S - T)
        text = ~aux["img_map"]
        assert torch.equal(img[2 * h:2 * h + 2, :Sh], aux["img_map"])
        assert torch.equal(pos[2 * h:2 * h + 2, :Sh].long(), o_pos.long()), side          # masked rows included
        got, want = x0[2 * h:2 * h + 2, :Sh][text], aux["merged"].bfloat16().float()[text]
        assert torch.equal(got, want), side                                              # text rows (padding included): the bf16 embedding row, or zeros
    # ---- values
    d_r = float(torch.cat([(rc.detach().cpu() - exp_c).abs(), (rr.detach().cpu() - exp_r).abs()]).max())
    d_l = abs(float(loss) - float(exp_loss))
    _record(f"{case:16s} rewards hip {[round(v, 5) for v in torch.cat([rc, rr]).tolist()]} oracle {[round(v, 5) for v in torch.cat([exp_c, exp_r]).tolist()]}")
    _record(f"{case:16s} max |reward - fp32 oracle| {d_r:.3e}   |loss - fp32 oracle| {d_l:.3e}   loss hip {float(loss):.5f} oracle {float(exp_loss):.5f}")
    emu_c, emu_r = R.rewards(W, cfg, rb, *R.rm_head(H), emulate=(EMU | {"vit"}) if "visual" in cfg else EMU)      # (a figure for the record, not a bound)
    d_e = float(torch.cat([(rc.detach().cpu() - emu_c).abs(), (rr.detach().cpu() - emu_r).abs()]).max())
    _record(f"{case:16s} max |reward - bf16-emulated oracle| {d_e:.3e}   (that oracle against its own fp32: "
            f"{float(torch.cat([(emu_c - exp_c).abs(), (emu_r - exp_r).abs()]).max()):.3e})")
    assert d_r < TOL_REWARD[case] and d_l < TOL_LOSS[case], (d_r, d_l)
    # ---- gradients
    loss.backward()
    torch.cuda.synchronize()
    named = dict(model.named_parameters())
    names, lm_head = _grad_names(cfg)
    # (the bias cancels in r_chosen - r_rejected: its gradient is zero in the oracle, and here up to the fp32 rounding of -a - b + a + b)
    assert float(exp_g["rm_head.bias"].abs()) < 1e-7 and float(named["rm_head.bias"].grad.float().abs()) < 1e-6
    pairs = [("rm_head.weight", named["rm_head.weight"].grad.view(-1), exp_g["rm_head.weight"])]
    pairs += [(n, named["base_model." + n].grad, exp_g[n]) for n in names]
    for n, got, want in pairs:
        cs, rm = cosine(got, want), relmax(got, want)
        print(f"[rm grads] {case} {n}: cosine {cs:.5f} relmax {rm:.3e}")
        assert cs > GRAD_COS and rm < GRAD_RELMAX, (n, cs, rm)
    # ---- the lm-head: in the graph with a zero gradient
    g_lm = named["base_model." + lm_head].grad
    assert float(g_lm.float().abs().sum()) == 0.0
    assert exp_g[lm_head] is None or float(exp_g[lm_head].abs().sum()) == 0.0
    o = _optim(cfg)
    lm0 = eng.policy.v["lm_head"].clone()
    head0 = torch.cat([t.clone() for t in eng.rm_head_views()[:2]])
    eng.optimizer_step(o["lr"], o["beta1"], o["beta2"], o["eps"], 0.0, o["max_grad_norm"])
    torch.cuda.synchronize()
    assert torch.equal(eng.policy.v["lm_head"], lm0)                                    # weight_decay 0: Adam's update of a zero gradient is 0
    assert not torch.equal(torch.cat(list(eng.rm_head_views()[:2])), head0)            # the head moved
    # ---- weight decay still applies to it: a second step on a fresh zero gradient, decay on
    lr, wd = 1e-2, 0.5
    master0 = eng.master[eng.layout.offset["lm_head"]: eng.layout.offset["lm_head"] + lm0.numel()].clone().view_as(lm0)
    bias0 = eng.rm_head_views()[1].clone()
    eng.zero_grad()
    loss2 = tr.compute_loss(model, tr._prepare_inputs(rb))
    loss2.backward()
    assert float(named["base_model." + lm_head].grad.float().abs().sum()) == 0.0
    eng.optimizer_step(lr, o["beta1"], o["beta2"], o["eps"], wd, o["max_grad_norm"])
    torch.cuda.synchronize()
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)      # noqa: E731
    two_roundings = (master0.cpu() * (f32(1.0) - f32(lr) * f32(wd))).bfloat16()         # w *= 1.f - lr * wd as written ...
    one_rounding = (master0.cpu() * f32(1.0 - float(f32(lr)) * float(f32(wd)))).bfloat16()      # ... or with the product contracted into an fma
    got = eng.policy.v["lm_head"].cpu()
    assert torch.equal(got, two_roundings) or torch.equal(got, one_rounding)
    assert not torch.equal(got, lm0.cpu())


# ------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("case", CASES)
def test_lora_trains_adapters_and_head_only(gpu, case):
    from vlrlhf.base.model import VLRewardModel
    cfg, W, rb, model, tr = build(case, lora=dict(PEFT, seed=5, modules_to_save=["rm_head"]))
    eng = model.engine
    assert tr.is_peft_model and isinstance(model, VLRewardModel) and "rm_head.w" in eng.lv
    w, b = R.rm_head(cfg["hidden"])
    assert torch.equal(eng.lv["rm_head.w"].cpu(), w.bfloat16()) and float(eng.lv["rm_head.b"]) == R.HEAD_BIAS      # the head moved into the adapters' buffer
    for k, t_ in eng.lv.items():                    # peft initialises B = 0: random B so that the adapters take part
        if ".b_" in k:
            t_.copy_(torch.randn(t_.shape, generator=torch.Generator().manual_seed(len(k))) * 0.02)
    eng.init_optimizer()
    base, ad = eng.policy.flat.clone(), eng.lora_flat.clone()
    loss = tr.training_step(model, rb)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    g = {k: float(v.float().abs().sum()) for k, v in eng.lgv.items()}
    g.pop("rm_head.b")                                                                # (zero by construction: the bias cancels in the pair loss)
    assert all(v > 0 for v in g.values()), [k for k, v in g.items() if v == 0]       # every adapter tensor and the head's weight
    assert model.rm_head.weight.grad.data_ptr() == eng.lgv["rm_head.w"].data_ptr()
    o = _optim(cfg)
    eng.optimizer_step(o["lr"], o["beta1"], o["beta2"], o["eps"], o["weight_decay"], o["max_grad_norm"])
    torch.cuda.synchronize()
    assert torch.equal(base, eng.policy.flat)                                          # every base weight bit-identical
    lo = eng.lora_layout
    assert not torch.equal(ad[: lo.offset["rm_head.w"]], eng.lora_flat[: lo.offset["rm_head.w"]])
    assert not torch.equal(ad[lo.offset["rm_head.w"]:], eng.lora_flat[lo.offset["rm_head.w"]:])
    if case == CASES[0]:
        with pytest.raises(NotImplementedError, match="modules_to_save"):
            build(case, lora=dict(PEFT, modules_to_save=["lm_head"]))


# ------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("case", CASES)
def test_score_save_load_and_eval_accuracy(gpu, case, tmp_path):
    cfg, W, rb, model, tr = build(case)
    exp_loss, exp_c, exp_r, _ = oracle(case)
    dev_rb = tr._prepare_inputs(rb)
    model.train()
    loss, out = tr.compute_loss(model, dev_rb, return_outputs=True)
    train_r = torch.cat([out["rewards_chosen"], out["rewards_rejected"]]).detach().clone()
    cb = tr.concatenated_inputs(dev_rb)
    scored = model.score(cb["input_ids"], cb["attention_mask"], reward_cols=cb["reward_cols"], **cb["img"])
    assert model.training and scored.shape == (4,) and not scored.requires_grad
    assert torch.equal(scored, train_r)                                 # eval mode, no grad: the training forward's rewards bit for bit
    # each half alone (the reference's two passes; reward column = the default, the last one) lands on the oracle within the same bound
    for side, exp in (("chosen", exp_c), ("rejected", exp_r)):
        alone = model.score(dev_rb[f"input_ids_{side}"], dev_rb[f"attention_mask_{side}"], **dev_rb["img_input_dict"])
        assert float((alone.cpu() - exp).abs().max()) < TOL_REWARD[case], side
    # rows with unequal image counts have no common reward column
    bad = cb["input_ids"].clone()
    tok = int(model.engine.cfg[model.image_count_key])
    bad[0][bad[0] == tok] = 1
    with pytest.raises(ValueError, match="same number of images"):
        model.score(bad, cb["attention_mask"], **cb["img"])
    # ---- save -> from_pretrained -> score
    out_dir = str(tmp_path / "rm")
    model.save_pretrained(out_dir)
    assert os.path.isfile(os.path.join(out_dir, "rm_head.bin")) and os.path.isfile(os.path.join(out_dir, "config.json"))
    sd = torch.load(os.path.join(out_dir, "rm_head.bin"))
    assert sd["weight"].shape == (1, cfg["hidden"]) and sd["bias"].shape == (1,)
    from vlrlhf.utils.auto_load import MyAutoRewardModel
    m2 = MyAutoRewardModel.from_pretrained(out_dir)
    assert torch.equal(m2.score(cb["input_ids"], cb["attention_mask"], reward_cols=cb["reward_cols"], **cb["img"]), train_r)
    # ---- eval accuracy: the fixture's pairs, then a head with a zero weight - every pair ties, and a tie counts as correct
    assert type(m2) is type(model)
    tr2 = type(tr)(m2, SimpleNamespace(per_device_eval_batch_size=2), lambda rows: rows[0], None, [rb], None)
    logs = tr2.evaluate()
    assert abs(logs["eval_accuracy"] - R.accuracy(exp_c, exp_r)) < 1e-6 and abs(logs["eval_loss"] - float(exp_loss)) < TOL_LOSS[case]
    m2.engine.set_rm_head(torch.zeros(cfg["hidden"]), torch.tensor([R.HEAD_BIAS]))
    logs = tr2.evaluate()
    ties = torch.full((2,), R.HEAD_BIAS)
    assert logs["eval_accuracy"] == R.accuracy(ties, ties) == 1.0 and abs(logs["eval_loss"] - float(R.pair_loss(ties, ties))) < 1e-6


# ------------------------------------------------------------------------------------------------------------ 4
def test_eight_step_trajectory_tracks_the_oracle_loop(gpu):
    """full fine-tune on the LLaVA fixture with the fixture's optimizer settings: every step's loss against the oracle loop computed the
    way the HIP path stores things (fp32 master weights, forward / backward on their bf16 rounding, restated clip + AdamW).  That the
    oracle's loss falls over these steps is checked on the CPU (tests/test_rm_host.py)."""
    case = CASES[0]
    cfg, W, rb, model, tr = build(case)
    o = _optim(cfg)
    eng = model.engine
    eng.init_optimizer()
    hip = []
    for _ in range(8):
        eng.zero_grad()
        hip.append(float(tr.training_step(model, rb)))
        eng.optimizer_step(o["lr"], o["beta1"], o["beta2"], o["eps"], o["weight_decay"], o["max_grad_norm"])
    torch.cuda.synchronize()
    w, b = R.rm_head(cfg["hidden"])
    ora = R.train_loop(W, cfg, rb, w, b, o, 8, emulate=EMU)
    worst = max(abs(h - r) for h, r in zip(hip, ora))
    _record("trajectory hip    " + " ".join(f"{x:.5f}" for x in hip))
    _record("trajectory oracle " + " ".join(f"{x:.5f}" for x in ora))
    _record(f"trajectory worst |hip - oracle| over 8 steps {worst:.3e}")
    assert hip[-1] < hip[0] and ora[-1] < ora[0]
    assert worst < TOL_TRAJECTORY, (hip, ora)


# ------------------------------------------------------------------------------------------------------------ 5
def _args(ckpt, out, **kw):
    a = dict(model_name_or_path=ckpt, dataset_name="synthetic", synthetic_rows=26, synthetic_image_size=28, output_dir=out,
             per_device_train_batch_size=2, max_steps=4, logging_steps=2, learning_rate=1e-4, max_length=64, warmup_ratio=0.0,
             lr_scheduler_type="constant", dataloader_prefetch=2, seed=3)
    a.update(kw)
    return [x for k, v in a.items() for x in (f"--{k}", str(v))]


def test_reward_modeling_main_end_to_end(gpu, tmp_path):
    """vlrlhf.reward_modeling.main on a tiny checkpoint and synthetic pairs: full fine-tune with checkpoints and evaluation, then LoRA -
    the files each leaves, and that what was written reloads to the trained bits"""
    from safetensors.torch import load_file
    from tests.golden_util import write_tiny_checkpoint
    from vlrlhf import reward_modeling as rm
    from vlrlhf.utils.auto_load import MyAutoRewardModel
    ckpt = str(tmp_path / "ckpt")
    write_tiny_checkpoint(ckpt)
    out = str(tmp_path / "full")
    tr = rm.main(_args(ckpt, out, save_strategy="steps", save_steps=2, save_total_limit=2, eval_strategy="steps", eval_steps=2,
                       gradient_accumulation_steps=2))
    hist = [h for h in tr.log_history if "loss" in h]
    assert len(hist) == 2 and hist[-1]["step"] == 4 and all(torch.isfinite(torch.tensor(h["loss"])) for h in hist)
    ev = [h for h in tr.log_history if "eval_loss" in h]
    assert ev and all(h["eval_accuracy"] in (0.0, 1.0) for h in ev)              # one eval pair (0.5 % of 26 rows, rounded up)
    for fn in ("checkpoint-4/trainer_state.json", "checkpoint-4/model.safetensors", "checkpoint-4/rm_head.bin",
               "checkpoint-4/optimizer_master.safetensors", "config.json", "model.safetensors", "rm_head.bin", "tokenizer.json", "trainer_state.json"):
        assert os.path.isfile(os.path.join(out, fn)), fn
    torch.cuda.synchronize()
    eng = tr.model.engine
    fresh, again = MyAutoRewardModel.from_pretrained(ckpt, seed=3), MyAutoRewardModel.from_pretrained(out)
    assert torch.equal(again.engine.policy.flat, eng.policy.flat)                # base weights and head (part of the flat buffer) reload to the trained bits
    w0, w1 = fresh.engine.rm_head_views()[0], again.engine.rm_head_views()[0]
    assert not torch.equal(w0, w1) and not torch.equal(fresh.engine.policy.flat, again.engine.policy.flat)      # and the head trained
    del tr, fresh, again
    out = str(tmp_path / "lora")
    tr = rm.main(_args(ckpt, out, use_lora="true", lora_r=8, lora_alpha=16, lora_dropout=0.0, max_steps=2, logging_steps=1,
                       save_strategy="steps", save_steps=2))
    sd = load_file(os.path.join(out, "adapter_model.safetensors"))
    assert all(".lora_A.weight" in k or ".lora_B.weight" in k for k in sd)       # the adapter file keeps the names save_adapter writes
    for fn in ("adapter_config.json", "rm_head.bin", "checkpoint-2/adapter_model.safetensors", "checkpoint-2/rm_head.bin"):
        assert os.path.isfile(os.path.join(out, fn)), fn
    head = torch.load(os.path.join(out, "rm_head.bin"))
    assert torch.equal(head["weight"].view(-1), tr.model.engine.lv["rm_head.w"].cpu()) and not torch.equal(head["weight"].view(-1), w0.cpu())
