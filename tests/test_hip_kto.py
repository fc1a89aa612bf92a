"""VLKTOTrainer on the MI355X (LLaVA-1.5 and Qwen-VL, full fine-tune and LoRA) against the CPU oracles: the fixture's two chosen rows are
the main rows of one KTO batch (labels desirable, undesirable), their KL rows are built by the KTO collator's own rule (prompt i, image i,
completion i - 1).  The policy's main-row log-probs bit for bit against a plain forward; ref / ref_kl / pi_kl against the fp32 oracle;
loss and kl against tests/kto_ref.py on the oracle's log-probs; one step's gradients against torch autograd through the oracle; the
reference pass through _reference_logps and the row-compact pass; evaluate(); vlrlhf.kto end to end in child processes, resumed to the
bits of the uninterrupted run; two optimizer steps of two accumulated minibatches against an oracle loop.
Needs a real MI355X:  pytest -m gpu"""
import functools
import json
import os
import shutil
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import kto_ref as KR  # noqa: E402
from tests.golden_util import load_case  # noqa: E402
from tests.test_hip_e2e import PEFT, TOL_LOGPS_FP32, cosine, gpu, relmax  # noqa: E402,F401  (the sequence-log-prob tolerance of the DPO tests)
from tests.test_hip_ppo import GRAD_COS, GRAD_RELMAX, _grad_names  # noqa: E402  (the bounds of tests/test_hip_grpo.py on one step's gradients)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("llava_hipsmall", "qwenvl_small")
BETA, W_D, W_U = 0.1, 1.25, 0.75
# (e) per-minibatch |HIP loss - oracle-loop loss| over 2 optimizer steps x 2 accumulated minibatches (losses of magnitude 0.5), measured on
# an MI355X against the fp32 oracle loop of tests/kto_ref.py train_steps (profiles/kto.txt, "trajectory") and doubled: the factor
# covers box-to-box bf16 differences (the margin rule of tests/test_hip_grpo.py).  Keys: (fixture, LoRA)
# measured 6.702e-4 / 6.901e-4 (full fine-tune, LLaVA / Qwen-VL) and 8.156e-4 / 1.639e-3 (LoRA, random B, learning rate 1e-4); 1 box, 1 run
TOL_TRAJECTORY = {("llava_hipsmall", False): 1.3404e-3, ("qwenvl_small", False): 1.3802e-3, ("llava_hipsmall", True): 1.6312e-3,
                  ("qwenvl_small", True): 3.2784e-3}


def _record(line):
    f = os.environ.get("VLR_KTO_MARGINS")
    print(line)
    if f:
        with open(f, "a") as fh:
            fh.write(line + "\n")


def kto_batch(batch, side="chosen", labels=(True, False)):
    """one side of the fixture's DPO batch -> a collated KTO batch: main rows = that side's rows, KL rows by
    VLKTODataCollatorWithPadding.kl_row"""
    from vlrlhf.base.collator import VLDPODataCollatorWithPadding, VLKTODataCollatorWithPadding
    rows, pad = [], 0
    for i in range(batch[f"{side}_input_ids"].shape[0]):
        L = int((batch[f"{side}_labels"][i] != -100).nonzero()[-1]) + 1      # the row without its right padding
        if L < batch[f"{side}_input_ids"].shape[1]:
            pad = int(batch[f"{side}_input_ids"][i, L])                     # the fixture's own pad id
        rows.append({f"completion_{k}": batch[f"{side}_{k}"][i, :L].tolist() for k in ("input_ids", "attention_mask", "labels")}
                    | dict(label=labels[i], img_path=f"img{i}"))
    out = VLKTODataCollatorWithPadding(VLDPODataCollatorWithPadding(pad, -100), max_length=4096, max_prompt_length=2048)(rows)
    for i, r in enumerate(rows):      # the main rows are the fixture's rows
        L = len(r["completion_input_ids"])
        assert out["chosen_input_ids"][i, :L].tolist() == r["completion_input_ids"] and bool((out["chosen_labels"][i, L:] == -100).all())
    out["img_input_dict"] = dict(pixel_values=batch["img_input_dict"]["pixel_values"])
    return out


def _pb(kb, half):
    return dict(input_ids=kb[f"{half}_input_ids"], attention_mask=kb[f"{half}_attention_mask"], labels=kb[f"{half}_labels"],
                pixel_values=kb["img_input_dict"]["pixel_values"])


@functools.lru_cache(maxsize=None)
def oracle_lora(case):
    """the oracle's adapters with a random B (so that the policy is not its own reference), on the bf16 grid; shared, never modified"""
    from oracle import llava_dpo_oracle as O
    from oracle import qwenvl_oracle as Q
    cfg = load_case(case)[1]
    lora = (Q if "visual" in cfg else O).random_lora(cfg, r=8, alpha=16, seed=3, b_std=0.05)
    lora["W"] = {k: v.bfloat16().float() for k, v in lora["W"].items()}
    return lora


def build(case, use_lora=False, **kw):
    from vlrlhf.base.trainer import KTOConfig
    from vlrlhf.models.Llava import LlavaForRL, LlavaKTOTrainer
    from vlrlhf.models.QwenVL import QwenVLForRL, QwenVLKTOTrainer
    z, cfg, W, W_ref, batch, _ = load_case(case)
    qwen = "visual" in cfg
    model = (QwenVLForRL if qwen else LlavaForRL).from_state_dict(cfg, W)
    ref = None
    if not use_lora:
        ref = (QwenVLForRL if qwen else LlavaForRL).from_state_dict(cfg, W_ref)
        ref.eval()
    a = dict(beta=BETA, desirable_weight=W_D, undesirable_weight=W_U, per_device_train_batch_size=2, learning_rate=1e-5, seed=3)
    a.update(kw)
    tr = (QwenVLKTOTrainer if qwen else LlavaKTOTrainer)(model, ref, KTOConfig(**a), peft_config=dict(PEFT, seed=5) if use_lora else None)
    if use_lora:
        assert tr.ref_model is None and tr.is_peft_model
        model.engine.load_lora_state_dict(oracle_lora(case)["W"])
        model.engine.init_optimizer()
    tr.keep_last = True
    return cfg, W, W_ref, batch, model, tr


@functools.lru_cache(maxsize=None)
def oracle(case, use_lora):
    """log-probs, loss and one step's gradients through the fp32 oracle, computed once per (fixture, LoRA) and shared.  Full fine-tune:
    the gradients of the decoder weights of _grad_names; LoRA: of every adapter, the reference being the adapter-free pass"""
    z, cfg, W, W_ref, batch, _ = load_case(case)
    kb = kto_batch(batch)
    lora = oracle_lora(case) if use_lora else None
    src = lora["W"] if use_lora else W
    names = list(lora["W"]) if use_lora else _grad_names(cfg)
    leaves = {k: src[k].clone().requires_grad_(True) for k in names}
    Wl = dict(W)
    l2 = None
    if use_lora:
        l2 = dict(lora, W=leaves)
    else:
        Wl.update(leaves)
    total, st = KR.batch_loss(Wl, None if use_lora else W_ref, cfg, _pb(kb, "chosen"), _pb(kb, "rejected"), kb["kto_label"], BETA, W_D, W_U,
                              lora=l2, lora_nograd=lora)
    total.backward()
    return dict(st, grads={k: v.grad for k, v in leaves.items()})


def _hip_grad(named, name, use_lora):
    return named[name.replace(".weight", ".default.weight") if use_lora else name].grad


# ------------------------------------------------------------------------------------------------------------ (a) (b) (c) (d)
@pytest.mark.parametrize("use_lora", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_one_step_matches_oracle(gpu, case, use_lora):
    cfg, W, W_ref, batch, model, tr = build(case, use_lora)
    kb = kto_batch(batch)
    exp = oracle(case, use_lora)
    tag = f"{case}{' lora' if use_lora else ''}"
    loss = tr.training_step(model, kb)
    torch.cuda.synchronize()
    last = {k: v.float().cpu() for k, v in tr.last.items()}
    # (a) the policy's main-row log-probs are the bits of get_batch_logps on a plain forward of the same B rows
    model.train()
    pb = {k: v.cuda() for k, v in _pb(kb, "chosen").items()}
    with torch.no_grad():
        out = model(input_ids=pb["input_ids"], attention_mask=pb["attention_mask"], labels=pb["labels"], use_cache=False, pixel_values=pb["pixel_values"])
        plain = tr.get_batch_logps(out.logits, out.labels, average_log_prob=False, label_pad_token_id=-100)
    assert torch.equal(plain.float().cpu(), last["pi"])
    # (b) every log-prob against the fp32 oracle, within the sequence-log-prob tolerance of the DPO tests
    d = {k: float((last[k] - exp[k]).abs().max()) for k in ("pi", "ref", "ref_kl", "pi_kl")}
    _record(f"{tag:22s} max |logp - fp32 oracle| " + "  ".join(f"{k} {v:.3e}" for k, v in d.items()))
    assert all(v < TOL_LOGPS_FP32 for v in d.values()), d
    if use_lora:      # the adapters are live in both policy passes and off in the reference passes
        assert float((last["pi"] - last["ref"]).abs().max()) > 0 and float((last["pi_kl"] - last["ref_kl"]).abs().max()) > 0
    # (c) sigmoid' <= 1/4: |d loss_i| <= w beta / 4 (|d pi| + |d ref| + |d kl|), |d kl| <= 2 x the log-prob tolerance
    d_kl, d_loss = abs(float(last["stats"][1]) - exp["kl"]), abs(float(loss) - exp["loss"])
    _record(f"{tag:22s} loss hip {float(loss):.6f} oracle {exp['loss']:.6f} |diff| {d_loss:.3e}; kl hip {float(last['stats'][1]):.6f} oracle {exp['kl']:.6f} "
            f"|diff| {d_kl:.3e}")
    assert d_kl <= 2 * TOL_LOGPS_FP32 and d_loss <= max(W_D, W_U) * BETA / 4 * (4 * TOL_LOGPS_FP32)
    # the device's loss kernel on the device's own log-probs, its gradient included (upstream 1): within the derived bounds of its fp64 replay
    fails, _ = KR.check(last["losses"], last["rewards"], last["dpi"], last["stats"], last["pi"], last["ref"], kb["kto_label"], last["pi_kl"],
                        last["ref_kl"], BETA, W_D, W_U, 1.0)
    assert fails == [], fails
    assert float(last["stats"][6]) == 1.0 and float(last["stats"][7]) == 1.0 and float(loss) == float(last["stats"][0])
    assert float(last["dpi"][0]) < 0 < float(last["dpi"][1])      # the desirable row is pushed up, the undesirable one down
    # (d) the gradients of the step against torch autograd through the oracle
    named = dict(model.named_parameters())
    worst_c, worst_r = 1.0, 0.0
    for n, g in exp["grads"].items():
        hip = _hip_grad(named, n, use_lora)
        assert tuple(hip.shape) == tuple(g.shape), n
        cs, rm = cosine(hip, g), relmax(hip, g)
        worst_c, worst_r = min(worst_c, cs), max(worst_r, rm)
        assert cs > GRAD_COS and rm < GRAD_RELMAX, (n, cs, rm)
    _record(f"{tag:22s} gradients of {len(exp['grads'])} tensors against oracle autograd: worst cosine {worst_c:.5f}, worst relmax {worst_r:.3e}")
    # the stored metrics: DPO's way, the kernel's stat vector under their names
    m = tr._stored_metrics["train"]
    assert set(m) == {"rewards/chosen_sum", "rewards/rejected_sum", "logps/chosen_sum", "logps/rejected_sum", "count/chosen", "count/rejected", "kl"}
    assert float(m["logps/chosen_sum"][0]) == float(last["pi"][0]) and float(m["logps/rejected_sum"][0]) == float(last["pi"][1])


# ------------------------------------------------------------------------------------------------------------ (e)
@pytest.mark.parametrize("use_lora", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_trajectory_tracks_the_oracle_loop(gpu, case, use_lora):
    """two optimizer steps of two accumulated minibatches (the fixture's chosen rows labelled desirable / undesirable, its rejected rows
    labelled the other way round): every minibatch's loss against the fp32 oracle loop on the weights the HIP path stores (fp32 master,
    bf16 rounding per pass).  The loss
    function is called at upstream 1 and the loop's grad_scale applies 1 / gradient_accumulation_steps: the second step's losses depend
    on that scale"""
    lr = 1e-4 if use_lora else 2e-5
    cfg, W, W_ref, batch, model, tr = build(case, use_lora, gradient_accumulation_steps=2, learning_rate=lr)
    eng = model.engine
    mbs = [kto_batch(batch, "chosen", (True, False)), kto_batch(batch, "rejected", (False, True))]
    base = eng.policy.flat.clone()
    if eng.master is None:
        eng.init_optimizer()
    eng.zero_grad()
    hip, hip_norm = [], []
    for _ in range(2):
        for kb in mbs:
            hip.append(float(tr.training_step(model, kb)) * 2)      # training_step returns loss / gradient_accumulation_steps
        eng.optimizer_step(lr, 0.9, 0.999, 1e-8, 0.0, 1e9, grad_scale=0.5)      # (a clipping norm nothing reaches: the oracle loop does not clip)
        hip_norm.append(eng.grad_norm())
    torch.cuda.synchronize()
    assert eng.opt_step == 2 and (torch.equal(eng.policy.flat, base) if use_lora else not torch.equal(eng.policy.flat, base))
    ora, ora_norm = KR.train_steps(W, W_ref, cfg, [(_pb(kb, "chosen"), _pb(kb, "rejected"), kb["kto_label"]) for kb in mbs], BETA, W_D, W_U, 2, lr,
                                   emulate=False, lora=oracle_lora(case) if use_lora else None)
    worst = max(abs(h - o) for h, o in zip(hip, ora))
    tag = f"{case}{' lora' if use_lora else ''}"
    _record(f"{tag:22s} trajectory hip    " + " ".join(f"{x:.6f}" for x in hip))
    _record(f"{tag:22s} trajectory oracle " + " ".join(f"{x:.6f}" for x in ora))
    _record(f"{tag:22s} trajectory worst |hip - oracle| over 4 minibatches {worst:.3e}")
    _record(f"{tag:22s} trajectory gradient norms (the mean of the two minibatches' gradients) hip " + " ".join(f"{x:.5f}" for x in hip_norm)
            + "  oracle " + " ".join(f"{x:.5f}" for x in ora_norm))
    assert len(hip) == len(ora) == 4 and ora[2] != ora[0]      # the second step runs on moved weights
    # the scale of the accumulated gradient (Adam's update hides it): the norm the optimizer saw is that of the MEAN of the two
    # minibatches' gradients, within the 5 % tests/test_hip_e2e.py allows a step's gradient norm against oracle autograd
    assert all(abs(h - o) < 0.05 * o for h, o in zip(hip_norm, ora_norm)), (hip_norm, ora_norm)
    assert worst <= TOL_TRAJECTORY[(case, use_lora)], (hip, ora)


# ------------------------------------------------------------------------------------------------------------ (f)
def test_reference_pass_is_row_compact_where_dpo_gets_it(gpu):
    cfg, W, W_ref, batch, model, tr = build("llava_hipsmall")
    kb = kto_batch(batch)
    eng = tr.ref_model.engine
    eng.prefix_dedup_min_share = 0.0
    # a KTO training step goes through _reference_logps: its reference pass is the row-compact one
    n0 = eng.prefix_dedup_passes
    tr.training_step(model, kto_batch(batch))
    assert eng.prefix_dedup_passes == n0 + 1
    dev = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in kb.items() if k != "img_input_dict"}
    dev["img_input_dict"] = dict(pixel_values=kb["img_input_dict"]["pixel_values"].cuda())
    n0 = eng.prefix_dedup_passes
    on = torch.cat(tr._reference_logps(dict(dev))).float().cpu()      # (a fresh dict: the per-batch cache of the trainer is rebuilt)
    assert eng.prefix_dedup_passes > n0
    assert torch.equal(on, torch.cat([tr.last["ref"], tr.last["ref_kl"]]).float().cpu())      # the step's reference log-probs are these
    eng.prefix_dedup = False
    n1 = eng.prefix_dedup_passes
    off = torch.cat(tr._reference_logps(dict(dev))).float().cpu()
    assert eng.prefix_dedup_passes == n1
    assert float((on - off).abs().max()) < TOL_LOGPS_FP32


# ------------------------------------------------------------------------------------------------------------ (g)
def test_evaluate_reports_eval_metrics(gpu):
    cfg, W, W_ref, batch, model, tr = build("llava_hipsmall")
    kb = kto_batch(batch)
    tr.data_collator = lambda rows: rows[0]
    flat0 = model.engine.policy.flat.clone()
    out = tr.evaluate([kb, kb])      # the collator stub hands the collated batch over
    keys = {"eval_loss", "eval_kl", "eval_rewards/chosen_sum", "eval_rewards/rejected_sum", "eval_logps/chosen_sum", "eval_logps/rejected_sum",
            "eval_count/chosen", "eval_count/rejected"}
    assert keys <= set(out) and all(torch.isfinite(torch.tensor(float(out[k]))) for k in keys)
    assert out["eval_count/chosen"] == 1.0 and out["eval_count/rejected"] == 1.0 and torch.equal(model.engine.policy.flat, flat0)


# ------------------------------------------------------------------------------------------------------------ (h)
def _run_kto(args, limit=300):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "vl-rlhf_amd"), ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-m", "vlrlhf.kto", *[x for k, v in args.items() for x in (f"--{k}", str(v))]], capture_output=True,
                       text=True, timeout=limit, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def test_kto_main_trains_checkpoints_and_resumes(tmp_path):
    from safetensors.torch import load_file
    from tests.golden_util import write_tiny_checkpoint
    ckpt, out, out2 = str(tmp_path / "ckpt"), str(tmp_path / "out"), str(tmp_path / "out2")
    write_tiny_checkpoint(ckpt)
    a = dict(model_name_or_path=ckpt, dataset_name="synthetic_unpaired", synthetic_rows=26, synthetic_image_size=28, output_dir=out,
             per_device_train_batch_size=2, gradient_accumulation_steps=2, max_steps=4, logging_steps=1, learning_rate=1e-4, warmup_ratio=0.0, lr_scheduler_type="constant", seed=3, save_strategy="steps", save_steps=2, save_total_limit=4,
             beta=0.1, desirable_weight=1.0, undesirable_weight=1.33)
    _run_kto(a)
    for fn in ("checkpoint-2/trainer_state.json", "checkpoint-4/model.safetensors", "config.json", "model.safetensors", "trainer_state.json"):
        assert os.path.isfile(os.path.join(out, fn)), fn
    hist = [h for h in json.load(open(os.path.join(out, "trainer_state.json")))["log_history"] if "loss" in h]
    assert len(hist) == 4 and all({"loss", "kl", "rewards/chosen_sum", "count/chosen", "count/rejected"} <= set(h) for h in hist)
    assert all(torch.isfinite(torch.tensor(h["loss"])) for h in hist)
    trained, base = load_file(os.path.join(out, "model.safetensors")), load_file(os.path.join(ckpt, "model.safetensors"))
    assert any(not torch.equal(trained[k], base[k]) for k in base)
    # resumed from the checkpoint of step 2: the bits of the uninterrupted run - the loss of every later step and the trained weights
    os.makedirs(out2)
    shutil.copytree(os.path.join(out, "checkpoint-2"), os.path.join(out2, "checkpoint-2"))
    _run_kto(dict(a, output_dir=out2, resume_from_checkpoint="true"))
    hist2 = [h for h in json.load(open(os.path.join(out2, "trainer_state.json")))["log_history"] if "loss" in h]
    assert [h["loss"] for h in hist2] == [h["loss"] for h in hist] and [h["kl"] for h in hist2] == [h["kl"] for h in hist]
    again = load_file(os.path.join(out2, "model.safetensors"))
    assert all(torch.equal(again[k], trained[k]) for k in trained)
