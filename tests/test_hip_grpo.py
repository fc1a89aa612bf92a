"""token_logps on the plain family wrappers and the GRPO step on the MI355X (LLaVA-1.5 and Qwen-VL) against the CPU oracles
(tests/grpo_ref.py over tests/ppo_ref.py): the fixture's two chosen rows are split at the label boundary into (query, response), every
query gets G = 2 responses - the fixture's and a shortened one - with fixed scores.  Per-token log-probs; one step() with the whole batch
in one minibatch (old_logp = NULL: ratio exactly 1) - advantages, loss, every stat and the gradient against torch autograd through the
oracle; the accumulated gradient of two minibatches; trajectories of 2 steps x 2 iterations x 2 minibatches, full fine-tune and LoRA;
generate() over num_return_sequences; vlrlhf.grpo.main end to end with a reward function (a skipped batch, checkpoint and resume).
Needs a real MI355X:  pytest -m gpu"""
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import grpo_ref as GR  # noqa: E402
from tests.golden_util import load_case  # noqa: E402
from tests.test_hip_e2e import EMU, PEFT, cosine, gpu, relmax  # noqa: E402,F401
from tests.test_hip_ppo import GRAD_COS, GRAD_RELMAX, TOL_LOGP, _grad_names, _split  # noqa: E402  (the same forward, the same bounds)
from tests import ppo_ref as PR  # noqa: E402

CASES = ("llava_hipsmall", "qwenvl_small")
P, G = 2, 2
SCORES = (1.0, -0.5, 0.25, 2.0)
HP = dict(beta=0.04, epsilon=0.2, epsilon_high=0.28, loss_type="grpo", scale_rewards=True)
# max |HIP - fp32 oracle|, measured on an MI355X (profiles/grpo.txt) and doubled: the factor covers run-to-run kernel selection and a later
# compiler (the convention of tests/test_hip_ppo.py).  One step, the whole batch in one minibatch (LLaVA / Qwen-VL measured): loss
# 4.262e-6 / 2.948e-4 (the loss itself is 1.8e-4 / 2.0e-2: ratio = 1 leaves -mean(A) over each sequence and beta times the KL term), the
# token-mean of the KL term 9.538e-5 / 8.367e-3 (of 4.2e-3 / 0.48)
TOL_LOSS = {"llava_hipsmall": 8.53e-6, "qwenvl_small": 5.9e-4}
TOL_KL = {"llava_hipsmall": 1.91e-4, "qwenvl_small": 1.674e-2}
# per-minibatch |HIP loss - oracle-loop loss| over 2 steps x 2 iterations x 2 minibatches (losses of magnitude 1e-4 - 3e-2): measured
# 5.637e-4 / 1.352e-3, doubled the same way; under LoRA (random B, learning rate 1e-4) 9.127e-4 / 4.097e-3
TOL_TRAJECTORY = {"llava_hipsmall": 1.13e-3, "qwenvl_small": 2.71e-3}
TOL_LORA_TRAJECTORY = {"llava_hipsmall": 1.83e-3, "qwenvl_small": 8.2e-3}
# the first step's statistics of that trajectory (full fine-tune), per-minibatch figures averaged over its four minibatches as step()
# reports them, in the order of TRAJ_STAT_KEYS: measured (profiles/grpo.txt, "trajectory step 1 stats") 5.934e-5, 1.742e-4, 2.484e-4 /
# 5.538e-4, 1.520e-3, 1.216e-3 and doubled; the clip fractions are counts over the minibatch's tokens: where HIP and oracle clipped the
# same tokens the measured distance is 0 and so is the bound (compared with <=)
TRAJ_STAT_KEYS = {"grpo/loss": "loss", "grpo/kl": "kl", "grpo/ratio": "ratio", "grpo/clip_ratio/low": "clip_low", "grpo/clip_ratio/high": "clip_high",
                  "grpo/clip_ratio/region": "clip_region"}
TOL_TRAJ_STATS = {"llava_hipsmall": dict(zip(TRAJ_STAT_KEYS, (1.19e-4, 3.49e-4, 4.97e-4, 0.0, 0.0, 0.0))),
                  "qwenvl_small": dict(zip(TRAJ_STAT_KEYS, (1.108e-3, 3.04e-3, 2.44e-3, 0.0, 0.0, 0.0)))}


def _record(line):
    f = os.environ.get("VLR_GRPO_MARGINS")
    print(line)
    if f:
        with open(f, "a") as fh:
            fh.write(line + "\n")


def _group_rows(pb):
    """(queries [P], responses [P * G], the oracle's batch of the P * G rows): sample 0 of a query is the fixture's response, sample 1
    the same without its last two tokens (at least one stays)"""
    qs, rs = _split(pb)
    responses = [r for full in rs for r in (full, full[:max(1, full.numel() - 2)].clone())]
    n = len(responses)
    T = pb["input_ids"].shape[1]
    ids, mask, labels = torch.zeros(n, T, dtype=torch.long), torch.zeros(n, T, dtype=torch.long), torch.full((n, T), -100, dtype=torch.long)
    for i, r in enumerate(responses):
        q = qs[i // G]
        L = q.numel() + r.numel()
        ids[i, :L], mask[i, :L], labels[i, q.numel():L] = torch.cat([q, r]), 1, r
    px = pb["pixel_values"]
    img = [p for p in range(len(qs)) for _ in range(G)]
    return qs, responses, dict(input_ids=ids, attention_mask=mask, labels=labels, pixel_values=px[img])


def build(case, lora=None, **cfg_kw):
    from vlrlhf.base.trainer import GRPOConfig
    from vlrlhf.models.Llava import LlavaForRL, LlavaGRPOTrainer
    from vlrlhf.models.QwenVL import QwenVLForRL, QwenVLGRPOTrainer
    z, cfg, W, W_ref, batch, _ = load_case(case)
    qwen = "visual" in cfg
    model = (QwenVLForRL if qwen else LlavaForRL).from_state_dict(cfg, W)
    ref = None
    if lora is None:
        ref = (QwenVLForRL if qwen else LlavaForRL).from_state_dict(cfg, W_ref)
        ref.eval()
    else:
        model.apply_lora(lora)
    kw = dict(batch_size=P, num_generations=G, mini_batch_size=P * G, learning_rate=1e-5, beta=HP["beta"], epsilon=HP["epsilon"],
              epsilon_high=HP["epsilon_high"], loss_type=HP["loss_type"], scale_rewards=HP["scale_rewards"], seed=3)
    kw.update(cfg_kw)
    tr = (QwenVLGRPOTrainer if qwen else LlavaGRPOTrainer)(GRPOConfig(**kw), model, ref, None, None, None, None, None)
    tr.keep_rollout = True
    return cfg, W, PR.ppo_batch(batch), model, tr


@functools.lru_cache(maxsize=None)
def oracle(case):
    """one step with the whole batch in one minibatch through the fp32 oracle, computed once per fixture and shared (never modified)"""
    z, cfg, W, W_ref, batch, _ = load_case(case)
    _, _, pb4 = _group_rows(PR.ppo_batch(batch))
    names = _grad_names(cfg)
    out = GR.step_grads(W, W_ref, cfg, pb4, torch.tensor(SCORES), P, G, HP, [list(range(P * G))], names, 1.0)
    with torch.no_grad():
        out["tok"] = GR.token_logps(W, cfg, PR.ppo_batch(batch))[0]
    return out


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("case", CASES)
def test_token_logps_on_a_plain_wrapper_match_oracle(gpu, case):
    from vlrlhf.base.model import token_logps, token_seq_off
    cfg, W, pb, model, tr = build(case)
    assert not model.engine.cfg.get("v_head")
    exp = oracle(case)["tok"]
    model.eval()
    with torch.no_grad():
        tok = token_logps(model, pb["input_ids"].cuda(), pb["attention_mask"].cuda(), pb["labels"].cuda(), pixel_values=pb["pixel_values"].cuda())
    assert tok.dtype == torch.float32 and tok.shape == exp.shape
    lens = (pb["labels"][:, 1:] != -100).sum(-1).tolist()
    assert token_seq_off(model).tolist() == [0, lens[0], lens[0] + lens[1]]
    d = float((tok.cpu() - exp).abs().max())
    _record(f"{case:16s} max |token logp - fp32 oracle| {d:.3e}")
    assert d < TOL_LOGP[case], d
    with pytest.raises(ValueError, match="needs labels"):
        token_logps(model, pb["input_ids"].cuda(), pb["attention_mask"].cuda(), None, pixel_values=pb["pixel_values"].cuda())
    with pytest.raises(ValueError, match="no response token"):
        token_logps(model, pb["input_ids"].cuda(), pb["attention_mask"].cuda(), torch.full_like(pb["labels"], -100).cuda(),
                    pixel_values=pb["pixel_values"].cuda())


# ------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("case", CASES)
def test_one_step_matches_oracle(gpu, case):
    """P * G rows in one minibatch, one iteration: no old-log-prob pass runs (old_logp = NULL), the reference pass does (beta != 0)"""
    cfg, W, pb, model, tr = build(case, max_new_tokens=None)
    exp = oracle(case)
    qs, rs, pb4 = _group_rows(pb)
    flat0, ref0 = model.engine.policy.flat.clone(), tr.ref_model.engine.policy.flat.clone()
    stats = tr.step(qs, rs, list(SCORES), pixel_values=pb["pixel_values"])
    torch.cuda.synchronize()
    ro = tr.last_rollout
    assert ro["old_logp"] is None and ro["seq_off"] == exp["seq_off"] and len(ro["minibatch_stats"]) == 1 and model.engine.opt_step == 1
    d_ref = float((ro["ref_logp"].cpu() - exp["ref"]).abs().max())
    want = exp["stats"][0]
    d_loss, d_kl = abs(stats["grpo/loss"] - want["loss"]), abs(stats["grpo/kl"] - want["kl"])
    _record(f"{case:16s} step: max |ref logp - fp32 oracle| {d_ref:.3e}  loss {d_loss:.3e} (hip {stats['grpo/loss']:.6f} oracle {want['loss']:.6f})  "
            f"kl {d_kl:.3e} (hip {stats['grpo/kl']:.6f} oracle {want['kl']:.6f})")
    # the device's own arithmetic on the scores: the advantages kernel against its fp64 replay, within the derived bounds
    fails, _ = GR.check_advantages(ro["advantages"].cpu(), ro["adv_stats"].cpu(), torch.tensor(SCORES), P, G, HP["scale_rewards"])
    assert fails == [], fails
    # ---- stats: the keys, every one against the oracle
    keys = {"grpo/loss", "grpo/kl", "grpo/ratio", "grpo/clip_ratio/low", "grpo/clip_ratio/high", "grpo/clip_ratio/region", "grpo/reward_mean",
            "grpo/reward_std", "grpo/frac_reward_zero_std", "grpo/clipped_completions_frac", "tokens/queries_len_mean", "tokens/responses_len_mean",
            "grpo/learning_rate"}
    assert set(stats) == keys and all(torch.isfinite(torch.tensor(v)) for v in stats.values())
    # the first minibatch with old_logp = NULL: exact
    assert stats["grpo/ratio"] == 1.0 and stats["grpo/clip_ratio/low"] == 0.0 and stats["grpo/clip_ratio/high"] == 0.0 and stats["grpo/clip_ratio/region"] == 0.0
    a = ro["adv_stats"].tolist()                              # (checked against the fp64 replay just above)
    assert (stats["grpo/reward_mean"], stats["grpo/reward_std"], stats["grpo/frac_reward_zero_std"]) == (a[0], a[1], 0.0)
    assert stats["grpo/clipped_completions_frac"] == 0.0 and stats["grpo/learning_rate"] == 1e-5
    assert stats["tokens/queries_len_mean"] == sum(q.numel() for q in qs) / P and stats["tokens/responses_len_mean"] == sum(r.numel() for r in rs) / (P * G)
    assert d_ref < TOL_LOGP[case] and d_loss <= TOL_LOSS[case] and d_kl <= TOL_KL[case], (d_ref, d_loss, d_kl)
    # the device's loss kernel on the device's own log-probs: nothing to compare here beyond the kernel tests, but the step's stat vector is
    # the kernel's (the keys name its entries)
    ms = ro["minibatch_stats"][0].tolist()
    assert (stats["grpo/loss"], stats["grpo/kl"], stats["grpo/ratio"]) == (ms[0], ms[1], ms[5]) and ms[6] == sum(r.numel() for r in rs) / (P * G)
    # ---- the gradient of the one minibatch (it stays in the gradient buffer after the optimizer step)
    named = dict(model.named_parameters())
    for n in _grad_names(cfg):
        cs, rm = cosine(named[n].grad, exp["grads"][n]), relmax(named[n].grad, exp["grads"][n])
        print(f"[grpo grads] {case} {n}: cosine {cs:.5f} relmax {rm:.3e}")
        assert cs > GRAD_COS and rm < GRAD_RELMAX, (n, cs, rm)
    assert not torch.equal(model.engine.policy.flat, flat0) and torch.equal(tr.ref_model.engine.policy.flat, ref0)
    # responses that ran to the length limit without a stop: with the limit at the longest response, that one row
    tr.config.max_new_tokens = max(r.numel() for r in rs)
    n_long = sum(r.numel() == tr.config.max_new_tokens for r in rs)
    tr.generation_kwargs = dict(eos_token_id=cfg["vocab"] - 1)
    assert tr._clipped_frac(rs) == n_long / (P * G)


@pytest.mark.parametrize("case", CASES)
def test_lora_first_minibatch_is_exact(gpu, case):
    """LoRA with fresh adapters (B = 0) and dropout 0: the policy IS the adapter-off reference, so the KL term is exactly 0 beside the
    exact ratio; only the adapters receive gradients and the base never moves"""
    cfg, W, pb, model, tr = build(case, lora=dict(PEFT, seed=5), learning_rate=1e-3)
    eng = model.engine
    assert tr.is_peft_model and tr.ref_model is None
    base, ad = eng.policy.flat.clone(), eng.lora_flat.clone()
    qs, rs, _ = _group_rows(pb)
    stats = tr.step(qs, rs, list(SCORES), pixel_values=pb["pixel_values"])
    torch.cuda.synchronize()
    assert stats["grpo/kl"] == 0.0 and stats["grpo/ratio"] == 1.0 and stats["grpo/clip_ratio/region"] == 0.0
    exp_ref = GR.token_logps(W, cfg, _group_rows(pb)[2])[0]               # the reference is the adapter-off pass of the policy's own base
    assert float((tr.last_rollout["ref_logp"].cpu() - exp_ref).abs().max()) < TOL_LOGP[case]
    assert torch.equal(base, eng.policy.flat) and not torch.equal(ad, eng.lora_flat)
    assert any(float(v.float().abs().sum()) > 0 for v in eng.lgv.values())


# ------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("case", CASES)
def test_accumulated_gradient_matches_oracle(gpu, case):
    """gradient_accumulation_steps = 2 over two minibatches of one group each: the gradient buffer after the step holds the SUM of the two
    minibatches' gradients, each with upstream 1 / 2, both at the step's weights (one optimizer step, after both; old_logp = NULL)"""
    cfg, W, pb, model, tr = build(case, mini_batch_size=G, gradient_accumulation_steps=2)
    qs, rs, pb4 = _group_rows(pb)
    tr.step(qs, rs, list(SCORES), pixel_values=pb["pixel_values"])
    torch.cuda.synchronize()
    assert model.engine.opt_step == 1 and tr.last_rollout["old_logp"] is None and len(tr.last_rollout["minibatch_stats"]) == 2
    z, _, _, W_ref, _, _ = load_case(case)
    names = _grad_names(cfg)
    mbs = [list(range(0, G)), list(range(G, 2 * G))]
    exp = GR.step_grads(W, W_ref, cfg, pb4, torch.tensor(SCORES), P, G, HP, mbs, names, 0.5)["grads"]
    one = GR.step_grads(W, W_ref, cfg, pb4, torch.tensor(SCORES), P, G, HP, mbs[1:], names, 0.5)["grads"]
    named = dict(model.named_parameters())
    for n in names:
        got = named[n].grad.reshape(-1)
        cs, rm = cosine(got, exp[n].reshape(-1)), relmax(got, exp[n].reshape(-1))
        print(f"[grpo accumulated grads] {case} {n}: cosine {cs:.5f} relmax {rm:.3e}   (the last minibatch alone: cosine {cosine(got, one[n].reshape(-1)):.5f})")
        assert cs > GRAD_COS and rm < GRAD_RELMAX, (n, cs, rm)
    assert cosine(named[names[0]].grad.reshape(-1), one[names[0]].reshape(-1)) < GRAD_COS      # the sum is not the last minibatch alone


# ------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("use_lora", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_trajectory_tracks_the_oracle_loop(gpu, case, use_lora):
    """2 steps x 2 iterations x 2 minibatches of one group: every minibatch's loss against the oracle loop computed the way the HIP path
    stores things (fp32 master weights, every pass on their bf16 rounding, restated Adam, generation order).  The rows see four optimizer
    steps per step(), so the old log-probs come from a no-grad pass: from the second minibatch on the ratio is not 1"""
    from oracle import qwenvl_oracle as Q
    from oracle import llava_dpo_oracle as O
    lr = 1e-4 if use_lora else 2e-5
    cfg, W, pb, model, tr = build(case, lora=dict(PEFT, seed=5) if use_lora else None, mini_batch_size=G, num_iterations=2, learning_rate=lr)
    lora = None
    if use_lora:
        lora = (Q if "visual" in cfg else O).random_lora(cfg, r=8, alpha=16, seed=3, b_std=0.05)
        lora["W"] = {k: v.bfloat16().float() for k, v in lora["W"].items()}
        model.engine.load_lora_state_dict(lora["W"])
        model.engine.init_optimizer()
        base = model.engine.policy.flat.clone()
    qs, rs, pb4 = _group_rows(pb)
    hip, first, first_ms = [], None, None
    for _ in range(2):
        stats = tr.step(qs, rs, list(SCORES), pixel_values=pb["pixel_values"])
        ms = tr.last_rollout["minibatch_stats"]
        assert tr.last_rollout["old_logp"] is not None and len(ms) == 4
        if first is None:
            first, first_ms = stats, torch.stack(ms).mean(0).tolist()
            assert float(ms[0][5]) == 1.0 and float(ms[0][4]) == 0.0 and float(ms[-1][5]) != 1.0      # the first minibatch sees its own numbers
        hip += [float(st[0]) for st in ms]
    torch.cuda.synchronize()
    assert model.engine.opt_step == 8
    if use_lora:
        assert torch.equal(model.engine.policy.flat, base)                  # the base never moves
    z, _, _, W_ref, _, _ = load_case(case)
    emu = (EMU | {"vit"}) if "visual" in cfg else EMU
    o_stats = GR.train_steps(W, W_ref, cfg, pb4, torch.tensor(SCORES), P, G, HP, 2, 2, G, lr, emulate=emu, lora=lora)
    ora = [st["loss"] for st in o_stats]
    worst = max(abs(h - r) for h, r in zip(hip, ora))
    tag = "lora trajectory" if use_lora else "trajectory"
    _record(f"{case:16s} {tag} hip    " + " ".join(f"{x:.6f}" for x in hip))
    _record(f"{case:16s} {tag} oracle " + " ".join(f"{x:.6f}" for x in ora))
    _record(f"{case:16s} {tag} worst |hip - oracle| over 8 minibatches {worst:.3e}")
    want = {k: sum(st[e] for st in o_stats[:4]) / 4 for k, e in TRAJ_STAT_KEYS.items()}
    dist = {k: abs(first[k] - want[k]) for k in TRAJ_STAT_KEYS}
    _record(f"{case:16s} {tag} step 1 stats |hip - oracle|: " + "  ".join(f"{k} {v:.3e} (oracle {want[k]:.5f})" for k, v in dist.items()))
    assert len(hip) == len(ora) == 8 and any(st["ratio"] != 1.0 for st in o_stats)
    assert worst <= (TOL_LORA_TRAJECTORY if use_lora else TOL_TRAJECTORY)[case], (hip, ora)
    if not use_lora:
        for k, e in TRAJ_STAT_KEYS.items():
            assert dist[k] <= TOL_TRAJ_STATS[case][k], (k, first[k], want[k])
            assert first[k] == first_ms[GR.STAT_NAMES.index(e)], k         # the key reports the kernel's entry of that name, exactly


# ------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("case", CASES)
def test_generate_returns_groups_in_repeat_interleave_order(gpu, case):
    """generate(): P * G rows from ONE call of the model's generate, row p * G + j continuing prompt p; under top_k = 1 sampling is greedy, so
    the G rows of a group are equal and begin with the greedy first token of their prompt; each row is cut after its first stop"""
    cfg, W, pb, model, tr = build(case, num_generations=3, mini_batch_size=6, max_new_tokens=5)
    qs, _ = _split(pb)
    px = pb["pixel_values"]
    calls = []
    inner = model.generate
    model.generate = lambda *a, **k: (calls.append(k), inner(*a, **k))[1]
    kw = dict(top_k=1, eos_token_id=cfg["vocab"] - 1, pad_token_id=0)      # an id greedy decoding does not reach here
    was = model.training
    rows = tr.generate(qs, generation_kwargs=kw, pixel_values=px)
    assert len(calls) == 1 and calls[0]["do_sample"] is True and calls[0]["num_return_sequences"] == 3 and calls[0]["max_new_tokens"] == 5
    assert model.training == was and len(rows) == 6 and all(r.dtype == torch.long and r.device.type == "cpu" and r.numel() == 5 for r in rows)
    for p in range(2):
        assert all(torch.equal(rows[3 * p + j], rows[3 * p]) for j in range(3)), p
    # the first token of group p is the greedy first token of prompt p (the prefill of the same left-padded batch)
    T0 = max(q.numel() for q in qs)
    ids, mask = torch.zeros(2, T0, dtype=torch.long), torch.zeros(2, T0, dtype=torch.long)
    for i, q in enumerate(qs):
        ids[i, T0 - q.numel():], mask[i, T0 - q.numel():] = q, 1
    greedy = inner(input_ids=ids.cuda(), attention_mask=mask.cuda(), pixel_values=px.cuda(), max_new_tokens=1, do_sample=False,
                   eos_token_id=cfg["vocab"] - 1, pad_token_id=0).cpu()
    assert [int(rows[3 * p][0]) for p in range(2)] == [int(greedy[p, T0]) for p in range(2)]
    # a stop: the third token of group 0 as eos - every row ends WITH its first occurrence
    stop = int(rows[0][2])
    cut = tr.generate(qs, generation_kwargs=dict(kw, eos_token_id=stop), pixel_values=px)

    def upto(row):
        return row[: row.index(stop) + 1] if stop in row else row
    assert [c.tolist() for c in cut] == [upto(r.tolist()) for r in rows] and int(cut[0][-1]) == stop and cut[0].numel() <= 3
    # sampling for real: the trainer's own generator drives it - two trainers with one seed draw the same rows
    free = tr.generate(qs, generation_kwargs=dict(eos_token_id=cfg["vocab"] - 1, pad_token_id=0), pixel_values=px)
    tr2 = build(case, num_generations=3, mini_batch_size=6, max_new_tokens=5)[4]
    tr._sample_gen.manual_seed(11)
    tr2._sample_gen.manual_seed(11)
    a = tr.generate(qs, generation_kwargs=dict(eos_token_id=cfg["vocab"] - 1, pad_token_id=0), pixel_values=px)
    b = tr2.generate(qs, generation_kwargs=dict(eos_token_id=cfg["vocab"] - 1, pad_token_id=0), pixel_values=px)
    assert len(free) == 6 and all(torch.equal(x, y) for x, y in zip(a, b))
    # what generate returns is what step() takes
    stats = tr.step(qs, cut, [0.5, 1.0, -1.0, 0.0, 2.0, 2.0], pixel_values=px)
    assert all(torch.isfinite(torch.tensor(v)) for v in stats.values())


# ------------------------------------------------------------------------------------------------------------ 6
def _grpo_args(ckpt, out, **kw):
    a = dict(model_name_or_path=ckpt, dataset_name="synthetic_queries", synthetic_rows=5, synthetic_image_size=28, output_dir=out, batch_size=2,
             num_generations=2, mini_batch_size=2, num_iterations=2, learning_rate=1e-4, max_new_tokens=4, seed=3, save_steps=1)
    a.update(kw)
    return [x for k, v in a.items() for x in (f"--{k}", str(v))]


def _reward(queries, responses):
    """a rule-based reward: longer answers with more distinct characters score higher"""
    return [0.1 * len(r) + 0.5 * len(set(r)) for r in responses]


def test_grpo_main_trains_skips_checkpoints_and_resumes(gpu, tmp_path):
    """vlrlhf.grpo.main on a tiny checkpoint, synthetic queries and a reward function: two batches of the real generate -> decode -> score ->
    step; then a batch whose scoring raises is skipped; then a run resumed from the first checkpoint lands on the bits of the
    uninterrupted one - sampling included, whose generator is part of the checkpoint"""
    from tests.golden_util import write_tiny_checkpoint
    from vlrlhf import grpo
    from vlrlhf.utils.auto_load import MyAutoModel
    ckpt, out = str(tmp_path / "ckpt"), str(tmp_path / "out")
    write_tiny_checkpoint(ckpt)
    fresh = MyAutoModel.from_pretrained(ckpt)
    flat0 = fresh.engine.policy.flat.clone()
    del fresh
    seen = []

    def reward(queries, responses):
        seen.append((list(queries), list(responses)))
        return _reward(queries, responses)
    tr = grpo.main(_grpo_args(ckpt, out), reward_fn=reward)
    torch.cuda.synchronize()
    eng = tr.model.engine
    assert tr.state.global_step == 2 and len(tr.log_history) == 2 and tr.last_rollout is None and eng.opt_step == 8
    assert len(seen) == 2 and all(len(q) == len(r) == 4 and q[0] == q[1] and q[2] == q[3] and q[0] != q[2] for q, r in seen)      # row p * G + j carries query p
    for h in tr.log_history:
        assert all(torch.isfinite(torch.tensor(v)) for k, v in h.items() if k.startswith(("grpo/", "tokens/")))
        assert len(h["game_log"]) == 2 and all("<image>" not in g["query"] and isinstance(g["response"], str) for g in h["game_log"])
        assert 1 <= h["tokens/responses_len_mean"] <= 4
    assert abs(tr.log_history[0]["grpo/reward_mean"] - sum(_reward(*seen[0])) / 4) < 1e-5
    assert not torch.equal(eng.policy.flat, flat0) and torch.equal(tr.ref_model.weights.flat, flat0)      # the policy moved, the frozen copy did not
    for fn in ("checkpoint-1/trainer_state.json", "checkpoint-1/model.safetensors", "checkpoint-1/optimizer_master.safetensors",
               "checkpoint-2/trainer_state.json", "config.json", "model.safetensors", "tokenizer.json"):
        assert os.path.isfile(os.path.join(out, fn)), fn
    final_flat, final_gen = eng.policy.flat.clone(), tr._sample_gen.get_state().clone()
    again = MyAutoModel.from_pretrained(out)
    assert torch.equal(again.engine.policy.flat, final_flat)                # what was written reloads to the trained bits
    del again
    # ---- a batch whose scoring raises is skipped: no step for it, the next batch runs
    calls = {"n": 0}

    def flaky(queries, responses):
        calls["n"] += 1
        if calls["n"] == 1:
            raise RuntimeError("scoring failed")
        return _reward(queries, responses)
    tr.reward_fn = flaky
    tr.config.save_steps = 0
    tr.train()
    assert calls["n"] == 2 and tr.skipped_batches == 1 and tr.state.global_step == 3 and len(tr.log_history) == 3
    del tr
    # ---- resume from the first checkpoint: the second batch alone, to the same bits
    tr2 = grpo.main(_grpo_args(ckpt, str(tmp_path / "out2"), resume_from_checkpoint=os.path.join(out, "checkpoint-1"), save_steps=0), reward_fn=_reward)
    torch.cuda.synchronize()
    assert tr2.state.global_step == 2 and len(tr2.log_history) == 2 and tr2.model.engine.opt_step == 8
    assert torch.equal(tr2._sample_gen.get_state(), final_gen)
    assert torch.equal(tr2.model.engine.policy.flat, final_flat)
