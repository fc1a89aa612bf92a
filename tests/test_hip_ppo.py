"""The PPO policy with its value head and the PPO step on the MI355X (LLaVA-1.5 and Qwen-VL) against the CPU oracles (tests/ppo_ref.py): the
fixture's chosen rows are split at the label boundary into (query, response), the scores are fixed numbers.  Per-token log-probs and
values of the policy pass; one step() with mini_batch_size = batch_size and ppo_epochs = 1 - advantages, returns, loss, stats and the
gradients against torch autograd through the oracle; what the first minibatch owes (policykl and ratio - 1); LoRA with the head trained
beside the adapters and the adapter-off reference; trajectories of 2 steps x 2 epochs x 2 minibatches against the oracle loop, full
fine-tune and LoRA; the KL controller; the save / load round trip of the head in both layouts; generate(); vlrlhf.ppo.main end to end
(generate, score with a reward model, step, a skipped batch, checkpoint and resume); the q_lora refusal.
Needs a real MI355X:  pytest -m gpu"""
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import llava_dpo_oracle as O  # noqa: E402  (checker only)
from tests import ppo_ref as PR  # noqa: E402
from tests.golden_util import load_case  # noqa: E402
from tests.test_hip_e2e import EMU, PEFT, cosine, gpu, relmax  # noqa: E402,F401
from tests.test_hip_ppo_kernels import U, _mean_bound, adv_bounds  # noqa: E402  (the derived fp32 bounds of the kernels)

CASES = ("llava_hipsmall", "qwenvl_small")
SCORES = (1.0, -0.5)
HP = dict(kl_coef=0.2, kl_penalty="kl", gamma=1.0, lam=0.95, whiten_rewards=False, cliprange=0.2, cliprange_value=0.2, vf_coef=0.1,
          ratio_threshold=10.0)
# max |HIP - fp32 oracle|, measured on an MI355X (profiles/ppo.txt) and doubled: the factor covers run-to-run kernel selection and a later
# compiler (the convention of tests/test_hip_rm.py).  Measured (LLaVA / Qwen-VL): token log-probs 1.927e-2 / 5.076e-2 (policy; the
# reference pass 1.382e-2 / 4.492e-2), values 1.421e-2 / 2.488e-2, whitened advantages 2.715e-2 / 2.224e-2, returns 1.239e-2 / 1.164e-2,
# total loss 1.496e-5 / 2.723e-4 (the loss itself is 7.1e-3 / 5.3e-2: ratio = 1 in the first minibatch leaves -mean(A) = 0 and the value
# term).  For scale, the oracle's own bf16 emulation of the decoder (O.HIP_ROUNDING; + the vision tower for Qwen-VL) sits 1.854e-2 /
# 5.564e-2 (log-probs) and 9.096e-3 / 2.826e-2 (values) from its fp32 on the same rows: the HIP path is of that order.
TOL_LOGP = {"llava_hipsmall": 3.86e-2, "qwenvl_small": 1.016e-1}
TOL_VALUE = {"llava_hipsmall": 2.85e-2, "qwenvl_small": 4.98e-2}
TOL_ADV = {"llava_hipsmall": 5.43e-2, "qwenvl_small": 4.45e-2}
TOL_RET = {"llava_hipsmall": 2.48e-2, "qwenvl_small": 2.33e-2}
TOL_LOSS = {"llava_hipsmall": 3.0e-5, "qwenvl_small": 5.45e-4}
# per-minibatch |HIP total loss - oracle-loop loss| over 2 steps x 2 epochs x 2 minibatches (losses of magnitude 0.4 - 1.2): measured
# 1.699e-3 / 1.754e-2, doubled the same way
TOL_TRAJECTORY = {"llava_hipsmall": 3.4e-3, "qwenvl_small": 3.51e-2}
# |stat of step() - the oracle's| for the statistics that are neither exact nor covered above, measured and doubled the same way.
# One step, one minibatch of the whole batch (LLaVA / Qwen-VL measured): objective/kl 2.372e-2 / 2.399e-2, mean_non_score_reward 3.388e-4 /
# 5.050e-4, loss/value 1.496e-4 / 2.724e-3, returns/mean 6.296e-3 / 8.183e-4, returns/var 1.205e-3 / 1.426e-3, val/vpred = val/mean
# 6.184e-3 / 6.467e-3, val/error 2.993e-4 / 5.447e-3, val/var 1.484e-4 / 2.130e-3
STAT_KEYS = {"objective/kl": ("adv", 0), "ppo/mean_non_score_reward": ("adv", 1), "ppo/loss/value": "vf",
             "ppo/returns/mean": "returns_mean", "ppo/returns/var": "returns_var", "ppo/val/vpred": "vpred_mean", "ppo/val/error": "error",
             "ppo/val/mean": "values_mean", "ppo/val/var": "values_var"}
TOL_STATS = {"llava_hipsmall": dict(zip(STAT_KEYS, (4.75e-2, 6.78e-4, 3.0e-4, 1.26e-2, 2.41e-3, 1.24e-2, 5.99e-4, 1.24e-2, 2.97e-4))),
             "qwenvl_small": dict(zip(STAT_KEYS, (4.8e-2, 1.01e-3, 5.45e-3, 1.64e-3, 2.86e-3, 1.3e-2, 1.09e-2, 1.3e-2, 4.26e-3)))}
# the same for a step of 2 epochs x 2 minibatches of one row (the first step of the trajectory test), where the policy has moved: every
# per-minibatch statistic, averaged over the four minibatches as step() reports it, against the oracle loop's
TRAJ_STAT_KEYS = {"ppo/loss/policy": "pg", "ppo/loss/value": "vf", "ppo/loss/total": "loss", "ppo/policy/approxkl": "approxkl",
                  "ppo/policy/policykl": "policykl", "ppo/policy/clipfrac": "pg_clipfrac", "ppo/policy/advantages_mean": "advantages_mean",
                  "ppo/policy/ratio": "ratio", "ppo/returns/mean": "returns_mean", "ppo/returns/var": "returns_var", "ppo/val/vpred": "vpred_mean",
                  "ppo/val/error": "error", "ppo/val/clipfrac": "vf_clipfrac", "ppo/val/mean": "values_mean", "ppo/val/var": "values_var"}
# measured (profiles/ppo.txt, "trajectory step 1 stats") and doubled, in the order of TRAJ_STAT_KEYS; the clip fractions are counts over the
# minibatch's tokens: where HIP and oracle clipped the same tokens the measured distance is 0 and so is the bound (compared with <=)
TOL_TRAJ_STATS = {"llava_hipsmall": dict(zip(TRAJ_STAT_KEYS, (2.8e-4, 6.24e-4, 2.18e-4, 2.34e-5, 7.04e-4, 0.0, 2.77e-4, 7.28e-4, 1.01e-2, 2.63e-4,
                                                               8.01e-3, 1.25e-3, 0.0, 6.39e-3, 4.96e-4))),
                  "qwenvl_small": dict(zip(TRAJ_STAT_KEYS, (8.95e-3, 8.64e-4, 8.87e-3, 2.16e-3, 4.38e-3, 1.131e-1, 1.77e-4, 2.08e-3, 1.34e-3, 8.48e-5,
                                                             1.273e-2, 1.73e-3, 0.0, 1.435e-2, 2.94e-3)))}
# the same under LoRA (adapters with random B and the head train, learning rate 1e-4): measured 2.166e-3 / 7.571e-3, doubled
TOL_LORA_TRAJECTORY = {"llava_hipsmall": 4.34e-3, "qwenvl_small": 1.515e-2}
GRAD_COS, GRAD_RELMAX = 0.995, 8e-2      # the bounds of tests/test_hip_sft.py on one step's gradients against oracle autograd


def _split(pb):
    """(queries, responses): every row cut at its first labelled token; the labels rebuilt from the cut are the fixture's"""
    qs, rs = [], []
    for ids, mask, lab in zip(pb["input_ids"], pb["attention_mask"], pb["labels"]):
        L, p = int(mask.sum()), int((lab != -100).nonzero()[0])
        assert bool((lab[p:L] == ids[p:L]).all()) and bool((lab[:p] == -100).all()) and bool((lab[L:] == -100).all())
        qs.append(ids[:p].clone())
        rs.append(ids[p:L].clone())
    return qs, rs


def build(case, lora=None, **cfg_kw):
    from vlrlhf.base.trainer import PPOConfig
    from vlrlhf.models.Llava import LlavaForRL, LlavaPPOTrainer, LlavaWithValueHead
    from vlrlhf.models.QwenVL import QwenVLForRL, QwenVLPPOTrainer, QwenVLWithValueHead
    z, cfg, W, W_ref, batch, _ = load_case(case)
    qwen = "visual" in cfg
    model = (QwenVLWithValueHead if qwen else LlavaWithValueHead).from_state_dict(cfg, W, v_head=PR.v_head(cfg["hidden"]))
    ref = None
    if lora is None:
        ref = (QwenVLForRL if qwen else LlavaForRL).from_state_dict(cfg, W_ref)
        ref.eval()
    else:
        model.apply_lora(lora)
    kw = dict(batch_size=2, mini_batch_size=2, ppo_epochs=1, learning_rate=1e-5, init_kl_coef=HP["kl_coef"], adap_kl_ctrl=True, target=6.0,
              horizon=100.0, gamma=HP["gamma"], lam=HP["lam"], cliprange=HP["cliprange"], cliprange_value=HP["cliprange_value"],
              vf_coef=HP["vf_coef"], kl_penalty=HP["kl_penalty"], whiten_rewards=HP["whiten_rewards"], seed=3)
    kw.update(cfg_kw)
    tr = (QwenVLPPOTrainer if qwen else LlavaPPOTrainer)(PPOConfig(**kw), model, ref, None, None, None, None, None)
    tr.keep_rollout = True                                                  # the tests read the step's rollout tensors
    return cfg, W, PR.ppo_batch(batch), model, tr


def _grad_names(cfg):
    """the last and the first decoder layer's q|k|v and down projections, the embedding, the lm-head"""
    L = cfg["layers"]
    if "visual" in cfg:
        per = lambda l: [f"transformer.h.{l}.attn.c_attn.weight", f"transformer.h.{l}.mlp.c_proj.weight"]      # noqa: E731
        return per(L - 1) + per(0) + ["transformer.wte.weight", "lm_head.weight"]
    p = "language_model.model.layers."
    per = lambda l: [f"{p}{l}.self_attn.{n}_proj.weight" for n in "qkv"] + [f"{p}{l}.mlp.down_proj.weight"]      # noqa: E731
    return per(L - 1) + per(0) + ["language_model.model.embed_tokens.weight", "language_model.lm_head.weight"]


@functools.lru_cache(maxsize=None)
def oracle(case):
    """the first minibatch of a step through the fp32 oracle, computed once per fixture and shared (and never modified)"""
    z, cfg, W, W_ref, batch, _ = load_case(case)
    w, b = PR.v_head(cfg["hidden"])
    names = [n for n in O.trainable_names(W) if not n.startswith("transformer.visual.")]
    return PR.minibatch_loss_and_grads(W, W_ref, cfg, PR.ppo_batch(batch), w, b, torch.tensor(SCORES), HP, names)


def _record(line):
    f = os.environ.get("VLR_PPO_MARGINS")
    print(line)
    if f:
        with open(f, "a") as fh:
            fh.write(line + "\n")


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("case", CASES)
def test_token_logps_and_values_match_oracle(gpu, case):
    cfg, W, pb, model, tr = build(case)
    exp = oracle(case)
    model.eval()
    with torch.no_grad():
        tok, none, values = model(pb["input_ids"].cuda(), pb["attention_mask"].cuda(), pb["labels"].cuda(), pixel_values=pb["pixel_values"].cuda())
    assert none is None and tok.dtype == values.dtype == torch.float32 and tok.shape == values.shape == exp["tok"].shape
    assert model.seq_off.tolist() == exp["seq_off"]
    d_l, d_v = float((tok.cpu() - exp["tok"]).abs().max()), float((values.cpu() - exp["values"]).abs().max())
    z, _, _, W_ref, batch, _ = load_case(case)
    emu = PR.policy_heads(W, cfg, pb, *PR.v_head(cfg["hidden"]), emulate=(EMU | {"vit"}) if "visual" in cfg else EMU)      # (a figure for the record, not a bound)
    _record(f"{case:16s} max |token logp - fp32 oracle| {d_l:.3e}  |value - fp32 oracle| {d_v:.3e}   (bf16-emulated oracle against its own fp32: "
            f"{float((emu[0] - exp['tok']).abs().max()):.3e} / {float((emu[1] - exp['values']).abs().max()):.3e})")
    assert d_l < TOL_LOGP[case] and d_v < TOL_VALUE[case], (d_l, d_v)
    # the lazy logits stand-in for callers that insist on [B, S, V]; no labels, no compact rows
    lg, _, v = model(pb["input_ids"].cuda(), pb["attention_mask"].cuda(), None, return_logits=True, pixel_values=pb["pixel_values"].cuda())
    assert v is None and tuple(lg.shape)[0] == 2 and tuple(lg.shape)[2] == cfg["vocab"]
    with pytest.raises(ValueError, match="needs labels"):
        model(pb["input_ids"].cuda(), pb["attention_mask"].cuda(), pixel_values=pb["pixel_values"].cuda())
    with pytest.raises(ValueError, match="no response token"):
        model(pb["input_ids"].cuda(), pb["attention_mask"].cuda(), torch.full_like(pb["labels"], -100).cuda(), pixel_values=pb["pixel_values"].cuda())


# ------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("case", CASES)
def test_one_step_matches_oracle_minibatch(gpu, case):
    cfg, W, pb, model, tr = build(case)
    exp = oracle(case)
    qs, rs = _split(pb)
    flat0 = model.engine.policy.flat.clone()
    ref0 = tr.ref_model.engine.policy.flat.clone()
    stats = tr.step(qs, rs, list(SCORES), pixel_values=pb["pixel_values"])
    torch.cuda.synchronize()
    ro = tr.last_rollout
    assert ro["seq_off"] == exp["seq_off"]
    d = {k: float((ro[k].cpu().double() - exp[e].double()).abs().max()) for k, e in
         (("old_logp", "tok"), ("old_values", "values"), ("ref_logp", "ref"), ("advantages", "advantages"), ("returns", "returns"))}
    d_loss = abs(stats["ppo/loss/total"] - exp["stats"]["loss"])
    _record(f"{case:16s} step: max |. - fp32 oracle| " + "  ".join(f"{k} {v:.3e}" for k, v in d.items()) + f"  loss {d_loss:.3e}"
            f"   (loss hip {stats['ppo/loss/total']:.5f} oracle {exp['stats']['loss']:.5f})")
    _record(f"{case:16s} first minibatch: policykl {stats['ppo/policy/policykl']:.3e}  ratio - 1 {stats['ppo/policy/ratio'] - 1:.3e}")
    assert d["old_logp"] < TOL_LOGP[case] and d["ref_logp"] < TOL_LOGP[case] and d["old_values"] < TOL_VALUE[case]
    assert d["advantages"] < TOL_ADV[case] and d["returns"] < TOL_RET[case] and d_loss < TOL_LOSS[case]
    # the device's own arithmetic on the device's rollout: the advantages kernel against its fp64 replay, within the bounds derived in
    # tests/test_hip_ppo_kernels.py from fp32 roundoff
    rep, bnd = adv_bounds(ro["old_logp"].cpu(), ro["ref_logp"].cpu(), ro["old_values"].cpu(), torch.tensor(ro["seq_off"]), torch.tensor(SCORES),
                          HP["kl_coef"], HP["kl_penalty"], HP["gamma"], HP["lam"], HP["whiten_rewards"])
    assert bool(((ro["advantages"].cpu().double() - rep["advantages"]).abs() <= bnd["advantages"]).all())
    assert bool(((ro["returns"].cpu().double() - rep["returns"]).abs() <= bnd["returns"]).all())
    # ---- stats: trl's keys, none of the entropy ones, every one against the oracle (a swapped index in step() shows here)
    keys = {"objective/kl", "objective/kl_coef", "ppo/loss/policy", "ppo/loss/value", "ppo/loss/total", "ppo/policy/approxkl", "ppo/policy/policykl",
            "ppo/policy/clipfrac", "ppo/policy/advantages_mean", "ppo/policy/ratio", "ppo/returns/mean", "ppo/returns/var", "ppo/val/vpred",
            "ppo/val/error", "ppo/val/clipfrac", "ppo/val/mean", "ppo/val/var", "ppo/mean_scores", "ppo/std_scores", "ppo/mean_non_score_reward",
            "tokens/queries_len_mean", "tokens/responses_len_mean", "ppo/learning_rate"}
    assert set(stats) == keys and all(torch.isfinite(torch.tensor(v)) for v in stats.values())
    want = {k: (float(exp["adv_stats"][e[1]]) if isinstance(e, tuple) else exp["stats"][e]) for k, e in STAT_KEYS.items()}
    dist = {k: abs(stats[k] - want[k]) for k in STAT_KEYS}
    _record(f"{case:16s} stats |hip - oracle|: " + "  ".join(f"{k} {v:.3e} (oracle {want[k]:.4f})" for k, v in dist.items()))
    for k in STAT_KEYS:
        assert dist[k] < TOL_STATS[case][k], (k, stats[k], want[k])
    # (with the whole batch in one minibatch val/vpred equals val/mean and loss/policy is -mean(A) = 0: the trajectory test tells those apart)
    # the first minibatch of the first epoch sees the rollout's own numbers: exact
    assert stats["ppo/policy/policykl"] == 0.0 and stats["ppo/policy/ratio"] == 1.0 and stats["ppo/policy/approxkl"] == 0.0
    assert stats["ppo/policy/clipfrac"] == 0.0 and stats["ppo/val/clipfrac"] == 0.0
    # the mean of the whitened advantages is 0 up to the fp32 sums (the kernel's mean bound, on the device's own advantages)
    A = ro["advantages"].cpu().double()
    b_mean = float(bnd["advantages"].mean()) + float(_mean_bound(A.abs().mean(), 0.0, A.numel())) + U
    assert abs(stats["ppo/policy/advantages_mean"]) <= b_mean and abs(stats["ppo/loss/policy"]) <= b_mean      # ratio = 1: the policy loss is -mean(A)
    assert stats["objective/kl_coef"] == HP["kl_coef"] and stats["ppo/mean_scores"] == 0.25 and stats["ppo/learning_rate"] == 1e-5
    assert abs(stats["ppo/std_scores"] - float(torch.tensor(SCORES).std())) < 1e-6
    assert stats["tokens/queries_len_mean"] == sum(q.numel() for q in qs) / 2 and stats["tokens/responses_len_mean"] == sum(r.numel() for r in rs) / 2
    # ---- the KL controller: kl_coef *= 1 + clip(kl / target - 1, -0.2, 0.2) * batch_size / horizon, from the logged KL
    e = min(max(stats["objective/kl"] / 6.0 - 1.0, -0.2), 0.2)
    assert abs(tr.kl_ctl.value - HP["kl_coef"] * (1.0 + e * 2 / 100.0)) < 1e-12
    # ---- gradients of the one minibatch (they stay in the gradient buffer after the optimizer step)
    named = dict(model.named_parameters())
    pairs = [("v_head.summary.weight", named["v_head.summary.weight"].grad.view(-1), exp["grads"]["v_head.summary.weight"]),
             ("v_head.summary.bias", named["v_head.summary.bias"].grad.view(-1), exp["grads"]["v_head.summary.bias"])]
    pairs += [(n, named["pretrained_model." + n].grad, exp["grads"][n]) for n in _grad_names(cfg)]
    for n, got, want in pairs:
        cs, rm = cosine(got, want), relmax(got, want)
        print(f"[ppo grads] {case} {n}: cosine {cs:.5f} relmax {rm:.3e}")
        assert cs > GRAD_COS and rm < GRAD_RELMAX, (n, cs, rm)
    # ---- the policy and the head moved, the reference did not
    assert not torch.equal(model.engine.policy.flat, flat0) and torch.equal(tr.ref_model.engine.policy.flat, ref0)
    off = model.engine.layout.offset["v_head.w"]
    assert not torch.equal(model.engine.policy.flat[off: off + cfg["hidden"]], flat0[off: off + cfg["hidden"]])


# ------------------------------------------------------------------------------------------------------------ 3
def test_two_epochs_two_minibatches_and_accumulation(gpu):
    """2 epochs x 2 minibatches of one row each: one optimizer step per backward batch; with gradient_accumulation_steps = 2 the two
    minibatches share one step and every gradient carries the 1 / 2 upstream.  Later minibatches see moved weights: policykl != 0."""
    case = CASES[0]
    for ga, steps in ((1, 4), (2, 2)):
        cfg, W, pb, model, tr = build(case, mini_batch_size=1, gradient_accumulation_steps=ga, ppo_epochs=2, learning_rate=1e-3)
        qs, rs = _split(pb)
        stats = tr.step(qs, rs, list(SCORES), pixel_values=pb["pixel_values"])
        torch.cuda.synchronize()
        assert model.engine.opt_step == steps and len(tr.last_rollout["minibatch_stats"]) == 4
        first, last = tr.last_rollout["minibatch_stats"][0].tolist(), tr.last_rollout["minibatch_stats"][-1].tolist()
        assert first[4] == 0.0 and first[7] == 1.0 and last[4] != 0.0 and last[7] != 1.0
        assert all(torch.isfinite(torch.tensor(v)) for v in stats.values())
    # the permutation generator is seeded by config.seed: two trainers draw the same order
    a = build(case, seed=9)[4]
    b = build(case, seed=9)[4]
    assert torch.randperm(8, generator=a._perm_gen).tolist() == torch.randperm(8, generator=b._perm_gen).tolist()


@pytest.mark.parametrize("case", CASES)
def test_accumulated_gradient_matches_oracle(gpu, case):
    """gradient_accumulation_steps = 2 over two minibatches of one row, one epoch: the gradient buffer after the step holds the SUM of
    the two minibatches' gradients, each with upstream 1 / 2, both at the rollout's weights (one optimizer step, after both) - against
    torch autograd through the oracle, the head included (vlr_v_head_bwd overwrites for the first minibatch and accumulates for the second)"""
    seed = 3
    cfg, W, pb, model, tr = build(case, mini_batch_size=1, gradient_accumulation_steps=2, ppo_epochs=1, seed=seed)
    qs, rs = _split(pb)
    tr.step(qs, rs, list(SCORES), pixel_values=pb["pixel_values"])
    torch.cuda.synchronize()
    assert model.engine.opt_step == 1
    perm = torch.randperm(2, generator=torch.Generator().manual_seed(seed)).tolist()
    z, _, _, W_ref, _, _ = load_case(case)
    names = _grad_names(cfg)
    exp = PR.accumulated_grads(W, W_ref, cfg, pb, *PR.v_head(cfg["hidden"]), torch.tensor(SCORES), HP, [[perm[0]], [perm[1]]], names, 0.5)
    one = PR.accumulated_grads(W, W_ref, cfg, pb, *PR.v_head(cfg["hidden"]), torch.tensor(SCORES), HP, [[perm[1]]], names, 0.5)
    named = dict(model.named_parameters())
    for n in ["v_head.summary.weight", "v_head.summary.bias"] + names:
        got = named[n if n.startswith("v_head.") else "pretrained_model." + n].grad
        cs, rm = cosine(got.reshape(-1), exp[n].reshape(-1)), relmax(got.reshape(-1), exp[n].reshape(-1))
        print(f"[ppo accumulated grads] {case} {n}: cosine {cs:.5f} relmax {rm:.3e}   (the last minibatch alone: cosine {cosine(got.reshape(-1), one[n].reshape(-1)):.5f})")
        assert cs > GRAD_COS and rm < GRAD_RELMAX, (n, cs, rm)
    # the sum is not the last minibatch alone: an overwrite in place of an accumulation would give that
    hw = named["v_head.summary.weight"].grad.reshape(-1)
    assert cosine(hw, one["v_head.summary.weight"].reshape(-1)) < GRAD_COS


@pytest.mark.parametrize("case", CASES)
def test_trajectory_tracks_the_oracle_loop(gpu, case):
    """full fine-tune, 2 steps x 2 epochs x 2 minibatches of one row: every minibatch's total loss against the oracle loop computed the way
    the HIP path stores things (fp32 master weights, every pass on their bf16 rounding, restated Adam, the same permutations), and the
    KL coefficient after each step against the controller formula on the logged KL.  The learning rate keeps every minibatch's mean ratio
    well under ratio_threshold (checked on the oracle: below half of it; at 1e-4 Adam drives the Qwen-VL fixture to 7.2 of the 10 in
    its third minibatch, where rounding decides whether the step is zeroed) while later minibatches still clip"""
    lr, seed = 2e-5, 3
    cfg, W, pb, model, tr = build(case, mini_batch_size=1, ppo_epochs=2, learning_rate=lr, seed=seed)
    qs, rs = _split(pb)
    hip, kls, coefs, first = [], [], [], None
    for _ in range(2):
        stats = tr.step(qs, rs, list(SCORES), pixel_values=pb["pixel_values"])
        if first is None:
            first, first_ms = stats, torch.stack(tr.last_rollout["minibatch_stats"]).mean(0).tolist()
        hip += [float(st[0]) for st in tr.last_rollout["minibatch_stats"]]
        kls.append(stats["objective/kl"])
        coefs.append(tr.kl_ctl.value)
    torch.cuda.synchronize()
    z, _, _, W_ref, _, _ = load_case(case)
    hp = dict(HP, target=6.0, horizon=100.0)
    emu = (EMU | {"vit"}) if "visual" in cfg else EMU
    o_stats, o_kls, o_coefs = PR.train_steps(W, W_ref, cfg, pb, *PR.v_head(cfg["hidden"]), torch.tensor(SCORES), hp, 2, 2, 1, lr, seed, emulate=emu)
    ora = [st["loss"] for st in o_stats]
    assert all(st["ratio"] < 0.5 * HP["ratio_threshold"] for st in o_stats) and any(st["pg_clipfrac"] > 0 for st in o_stats)
    worst = max(abs(h - r) for h, r in zip(hip, ora))
    _record(f"{case:16s} trajectory hip    " + " ".join(f"{x:.5f}" for x in hip))
    _record(f"{case:16s} trajectory oracle " + " ".join(f"{x:.5f}" for x in ora))
    _record(f"{case:16s} trajectory worst |hip - oracle| over 8 minibatches {worst:.3e}   kl hip {kls} oracle {o_kls}")
    assert len(hip) == len(ora) == 8 and all(x != 0.0 for x in ora)                    # (no minibatch trips the ratio threshold)
    assert worst < TOL_TRAJECTORY[case], (hip, ora)
    # ---- the first step's statistics, per-minibatch figures averaged over its four minibatches: each key against the oracle loop
    want = {k: sum(st[e] for st in o_stats[:4]) / 4 for k, e in TRAJ_STAT_KEYS.items()}
    dist = {k: abs(first[k] - want[k]) for k in TRAJ_STAT_KEYS}
    _record(f"{case:16s} trajectory step 1 stats |hip - oracle|: " + "  ".join(f"{k} {v:.3e} (oracle {want[k]:.4f})" for k, v in dist.items()))
    for k, e in TRAJ_STAT_KEYS.items():
        assert dist[k] <= TOL_TRAJ_STATS[case][k], (k, first[k], want[k])
        # and the key reports the entry of the kernel's stat vector that carries this quantity (the order tests/test_hip_ppo_kernels.py
        # checks against the fp64 replay) - exactly, so that two keys with close values cannot trade places unseen
        assert first[k] == first_ms[PR.STAT_NAMES.index(e)], k
    assert len({first_ms[PR.STAT_NAMES.index(e)] for e in TRAJ_STAT_KEYS.values() if "clipfrac" not in e}) == len(TRAJ_STAT_KEYS) - 2
    c = HP["kl_coef"]
    for kl, got in zip(kls, coefs):
        c *= 1.0 + min(max(kl / 6.0 - 1.0, -0.2), 0.2) * 2 / 100.0
        assert abs(got - c) < 1e-12
    assert abs(coefs[-1] - o_coefs[-1]) < 1e-3


@pytest.mark.parametrize("case", CASES)
def test_lora_trajectory_tracks_the_oracle_loop(gpu, case):
    """the same 2 steps x 2 epochs x 2 minibatches under LoRA: only the adapters (random B, so that they take part) and the head train, the
    reference is the adapter-off pass over the frozen base - every minibatch's total loss against the oracle loop with its adapter path"""
    from oracle import qwenvl_oracle as Q
    lr, seed = 1e-4, 3
    cfg, W, pb, model, tr = build(case, lora=dict(PEFT, seed=5), mini_batch_size=1, ppo_epochs=2, learning_rate=lr, seed=seed)
    lora = (Q if "visual" in cfg else O).random_lora(cfg, r=8, alpha=16, seed=3, b_std=0.05)
    lora["W"] = {k: v.bfloat16().float() for k, v in lora["W"].items()}
    eng = model.engine
    eng.load_lora_state_dict(lora["W"])
    eng.init_optimizer()
    base = eng.policy.flat.clone()
    qs, rs = _split(pb)
    hip, kls = [], []
    for _ in range(2):
        stats = tr.step(qs, rs, list(SCORES), pixel_values=pb["pixel_values"])
        hip += [float(st[0]) for st in tr.last_rollout["minibatch_stats"]]
        kls.append(stats["objective/kl"])
    torch.cuda.synchronize()
    assert torch.equal(eng.policy.flat, base)                               # the base never moves
    emu = (EMU | {"vit"}) if "visual" in cfg else EMU
    o_stats, o_kls, _ = PR.train_steps(W, None, cfg, pb, *PR.v_head(cfg["hidden"]), torch.tensor(SCORES), dict(HP, target=6.0, horizon=100.0),
                                       2, 2, 1, lr, seed, emulate=emu, lora=lora)
    ora = [st["loss"] for st in o_stats]
    assert all(st["ratio"] < 0.5 * HP["ratio_threshold"] for st in o_stats) and any(st["ratio"] != 1.0 for st in o_stats)
    worst = max(abs(h - r) for h, r in zip(hip, ora))
    _record(f"{case:16s} lora trajectory hip    " + " ".join(f"{x:.5f}" for x in hip))
    _record(f"{case:16s} lora trajectory oracle " + " ".join(f"{x:.5f}" for x in ora))
    _record(f"{case:16s} lora trajectory worst |hip - oracle| over 8 minibatches {worst:.3e}   kl hip {kls} oracle {o_kls}")
    assert len(hip) == len(ora) == 8 and worst < TOL_LORA_TRAJECTORY[case], (hip, ora)


def test_early_stopping_and_argument_errors(gpu):
    from vlrlhf.base.trainer import PPOConfig
    case = CASES[0]
    # trl decides once per epoch, on the policykl of the epoch's last minibatch, after the epoch's optimizer steps: with a target no
    # policykl can stay under (1.5 * -1e9) the first epoch runs whole - two minibatches, two optimizer steps - and no second one starts
    cfg, W, pb, model, tr = build(case, mini_batch_size=1, ppo_epochs=3, learning_rate=1e-5, early_stopping=True, target_kl=-1e9)
    qs, rs = _split(pb)
    flat0 = model.engine.policy.flat.clone()
    model.eval()                                                           # the caller's mode comes back after the step
    tr.step(qs, rs, list(SCORES), pixel_values=pb["pixel_values"])
    torch.cuda.synchronize()
    assert model.engine.opt_step == 2 and not torch.equal(model.engine.policy.flat, flat0) and len(tr.last_rollout["minibatch_stats"]) == 2
    assert not model.training and not model.pretrained_model.training
    model.train()
    tr.config.target_kl = 1e9                                              # never reached: all three epochs run
    tr.step(qs, rs, list(SCORES), pixel_values=pb["pixel_values"])
    assert model.engine.opt_step == 8 and len(tr.last_rollout["minibatch_stats"]) == 6 and model.training
    with pytest.raises(ValueError, match="batch_size"):
        tr.step(qs[:1], rs[:1], [0.0], pixel_values=pb["pixel_values"][:1])
    with pytest.raises(ValueError, match="scores"):
        tr.step(qs, rs, [0.0], pixel_values=pb["pixel_values"])
    with pytest.raises(ValueError, match="empty"):
        tr.step(qs, [rs[0], rs[1][:0]], list(SCORES), pixel_values=pb["pixel_values"])
    with pytest.raises(NotImplementedError, match="full"):
        type(tr)(PPOConfig(batch_size=2, mini_batch_size=2, kl_penalty="full"), model)
    with pytest.raises(NotImplementedError, match="more than one GPU"):
        type(tr)(PPOConfig(batch_size=2, mini_batch_size=2, world_size=2), model)
    with pytest.raises(ValueError, match="multiple"):
        PPOConfig(batch_size=3, mini_batch_size=2)


# ------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("case", CASES)
def test_lora_trains_adapters_and_head_only(gpu, case):
    cfg, W, pb, model, tr = build(case, lora=dict(PEFT, seed=5), learning_rate=1e-3)
    eng = model.engine
    assert tr.is_peft_model and tr.ref_model is None and "v_head.w" in eng.lv
    w, b = PR.v_head(cfg["hidden"])
    assert torch.equal(eng.lv["v_head.w"].cpu(), w.bfloat16()) and float(eng.lv["v_head.b"]) == PR.V_HEAD_BIAS      # the head moved into the adapters' buffer
    for k, t_ in eng.lv.items():                    # peft initialises B = 0: random B so that the adapters take part and the reference differs
        if ".b_" in k:
            t_.copy_(torch.randn(t_.shape, generator=torch.Generator().manual_seed(len(k))) * 0.02)
    eng.init_optimizer()
    base, ad = eng.policy.flat.clone(), eng.lora_flat.clone()
    qs, rs = _split(pb)
    stats = tr.step(qs, rs, list(SCORES), pixel_values=pb["pixel_values"])
    torch.cuda.synchronize()
    ro = tr.last_rollout
    assert not torch.equal(ro["old_logp"], ro["ref_logp"])                            # the reference is the adapter-off pass ...
    exp_ref = oracle(case)["tok"]                                                      # ... of the policy's own base weights
    assert float((ro["ref_logp"].cpu() - exp_ref).abs().max()) < TOL_LOGP[case]
    assert stats["objective/kl"] != 0.0 and stats["ppo/policy/policykl"] == 0.0
    g = {k: float(v.float().abs().sum()) for k, v in eng.lgv.items()}
    assert all(v > 0 for v in g.values()), [k for k, v in g.items() if v == 0]       # every adapter tensor and both head tensors
    assert model.v_head.summary.weight.grad.data_ptr() == eng.lgv["v_head.w"].data_ptr()
    assert torch.equal(base, eng.policy.flat)                                          # every base weight bit-identical
    lo = eng.lora_layout
    assert not torch.equal(ad[: lo.offset["v_head.w"]], eng.lora_flat[: lo.offset["v_head.w"]])
    assert not torch.equal(ad[lo.offset["v_head.w"]:], eng.lora_flat[lo.offset["v_head.w"]:])
    with pytest.raises(NotImplementedError, match="modules_to_save"):
        model.apply_lora(dict(PEFT, modules_to_save=["lm_head"]))


# ------------------------------------------------------------------------------------------------------------ 5
def test_value_head_save_load_round_trip_both_layouts(gpu, tmp_path):
    from vlrlhf.utils.auto_load import MyAutoModelWithValueHead
    case = CASES[0]
    cfg, W, pb, model, tr = build(case)
    args = (pb["input_ids"].cuda(), pb["attention_mask"].cuda(), pb["labels"].cuda())
    model.eval()
    with torch.no_grad():
        tok, _, values = model(*args, pixel_values=pb["pixel_values"].cuda())
    # ---- full fine-tune: the checkpoint + v_head.bin
    out = str(tmp_path / "full")
    model.save_pretrained(out)
    sd = torch.load(os.path.join(out, "v_head.bin"))
    assert sorted(sd) == ["v_head.summary.bias", "v_head.summary.weight"] and sd["v_head.summary.weight"].shape == (1, cfg["hidden"])
    m2 = MyAutoModelWithValueHead.from_pretrained(out)
    assert type(m2) is type(model) and m2.pretrained_model is not None
    m2.eval()
    with torch.no_grad():
        tok2, _, values2 = m2(*args, pixel_values=pb["pixel_values"].cuda())
    assert torch.equal(tok2, tok) and torch.equal(values2, values)
    names = [n for n, _ in m2.named_parameters()]
    assert names[-2:] == ["v_head.summary.weight", "v_head.summary.bias"] and all(n.startswith("pretrained_model.") for n in names[:-2])
    # a directory without a head file: a fresh head from the init strategy, the same for the same seed
    os.remove(os.path.join(out, "v_head.bin"))
    f1 = MyAutoModelWithValueHead.from_pretrained(out, v_head_init_strategy="normal", v_head_initializer_range=0.2, seed=4)
    f2 = MyAutoModelWithValueHead.from_pretrained(out, v_head_init_strategy="normal", v_head_initializer_range=0.2, seed=4)
    w1, b1 = f1.engine.v_head_views()[:2]
    assert torch.equal(w1, f2.engine.v_head_views()[0]) and float(b1) == 0.0 and 0.1 < float(w1.float().std()) < 0.3
    for bad in (dict(use_value_adapter=True), dict(reward_adapter="x")):
        with pytest.raises(NotImplementedError):
            MyAutoModelWithValueHead.from_pretrained(out, **bad)
    with pytest.raises(NotImplementedError, match="compute_reward_score"):
        f1.compute_reward_score(None)
    del m2, f1, f2
    # ---- LoRA: the adapter files + pytorch_model.bin holding exactly the two head tensors
    cfg, W, pb, model, tr = build(case, lora=dict(PEFT, seed=5))
    model.engine.set_v_head(torch.arange(cfg["hidden"]).float() / 64, torch.tensor([0.5]))
    out = str(tmp_path / "lora")
    model.save_pretrained(out)
    sd = torch.load(os.path.join(out, "pytorch_model.bin"))
    assert sorted(sd) == ["v_head.summary.bias", "v_head.summary.weight"]
    assert os.path.isfile(os.path.join(out, "adapter_model.safetensors")) and os.path.isfile(os.path.join(out, "adapter_config.json"))
    cfg, W, pb, m3, _ = build(case, lora=dict(PEFT, seed=6))
    m3.load_adapter(out)
    assert torch.equal(m3.engine.lora_flat, model.engine.lora_flat)                    # adapters and head reload to the saved bits
    assert float(m3.v_head.summary.bias.detach()) == 0.5


# ------------------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("case", CASES)
def test_generate_strips_prompt_and_tail_and_feeds_step(gpu, case):
    """generate(): left-padded queries of unequal length through the model's own generate, the prompt stripped, everything after the first
    stop token dropped (the stop kept); what it returns is what step() takes"""
    from types import SimpleNamespace
    cfg, W, pb, model, tr = build(case)
    qs, _ = _split(pb)
    qs = [qs[0], qs[1][1:]] if "visual" not in cfg else qs                # unequal lengths: the left padding is exercised (LLaVA: drop the BOS)
    px = pb["pixel_values"]
    T0 = max(q.numel() for q in qs)
    kw = dict(max_new_tokens=5, do_sample=False, eos_token_id=cfg["vocab"] - 1, pad_token_id=0)      # an id greedy decoding does not reach here
    was = model.training
    full = tr.generate(qs, generation_kwargs=kw, pixel_values=px)
    assert model.training == was and [r.numel() for r in full] == [5, 5] and all(r.dtype == torch.long and r.device.type == "cpu" for r in full)
    # the same rows straight from the model: left-padded ids, prompt + continuation
    ids = torch.zeros(2, T0, dtype=torch.long)
    mask = torch.zeros(2, T0, dtype=torch.long)
    for i, q in enumerate(qs):
        ids[i, T0 - q.numel():], mask[i, T0 - q.numel():] = q, 1
    raw = model.generate(input_ids=ids.cuda(), attention_mask=mask.cuda(), pixel_values=px.cuda(), **kw).cpu()
    assert raw.shape == (2, T0 + 5) and all(torch.equal(raw[i, T0:], full[i]) for i in range(2))
    def upto_stop(row, eos, seqs=()):
        """the row up to and including its first stop: an eos id, or the last token of a stop sequence"""
        for t in range(len(row)):
            if row[t] == eos or any(len(q) <= t + 1 and row[t + 1 - len(q): t + 1] == q for q in seqs):
                return row[: t + 1]
        return row

    # the third token of row 0 as eos: row 0 ends WITH its first occurrence, row 1 runs on unless it meets the same id
    stop = int(full[0][2])
    cut = tr.generate(qs, generation_kwargs=dict(kw, eos_token_id=stop), pixel_values=px)
    assert [c.tolist() for c in cut] == [upto_stop(f.tolist(), stop) for f in full] and int(cut[0][-1]) == stop and cut[0].numel() <= 3
    # a stop-word sequence of the generation config (tokens 2 and 3 of row 1): the row ends with the sequence's last token
    seq = full[1][1:3].tolist()
    gc = SimpleNamespace(stop_words_ids=[seq], max_new_tokens=5, do_sample=False, eos_token_id=cfg["vocab"] - 1, pad_token_id=0)
    by_word = tr.generate(qs, generation_kwargs=dict(generation_config=gc), pixel_values=px)
    assert [c.tolist() for c in by_word] == [upto_stop(f.tolist(), cfg["vocab"] - 1, [seq]) for f in full] and by_word[1].numel() <= 3
    # return_prompt: the query in front, and the trainer's default generation_kwargs are used when none are given
    tr.generation_kwargs = kw
    both = tr.generate(qs, return_prompt=True, pixel_values=px)
    assert all(torch.equal(both[i], torch.cat([qs[i], full[i]])) for i in range(2))
    stats = tr.step(qs, cut, list(SCORES), pixel_values=px)
    assert all(torch.isfinite(torch.tensor(v)) for v in stats.values()) and stats["tokens/responses_len_mean"] == (cut[0].numel() + cut[1].numel()) / 2


# ------------------------------------------------------------------------------------------------------------ 7
def _ppo_args(ckpt, rm_dir, out, **kw):
    a = dict(model_name_or_path=ckpt, reward_model_name_or_path=rm_dir, dataset_name="synthetic_queries", synthetic_rows=5,
             synthetic_image_size=28, output_dir=out, batch_size=2, mini_batch_size=2, ppo_epochs=1, learning_rate=1e-4, max_new_tokens=4,
             horizon=100.0, seed=3, save_steps=1)
    a.update(kw)
    return [x for k, v in a.items() for x in (f"--{k}", str(v))]


def test_ppo_main_trains_scores_skips_checkpoints_and_resumes(gpu, tmp_path, monkeypatch):
    """vlrlhf.ppo.main on a tiny checkpoint, synthetic queries and a reward model written by the reward-model classes: two batches of
    the real generate -> decode -> score -> step; then a batch whose scoring raises is skipped; then a run resumed from the first
    checkpoint lands on the bits of the uninterrupted one"""
    from tests.golden_util import write_tiny_checkpoint
    from vlrlhf import ppo
    from vlrlhf.utils.auto_load import MyAutoModelWithValueHead, MyAutoRewardModel
    ckpt, rm_dir, out = str(tmp_path / "ckpt"), str(tmp_path / "rm"), str(tmp_path / "out")
    write_tiny_checkpoint(ckpt)
    MyAutoRewardModel.from_pretrained(ckpt, seed=1).save_pretrained(rm_dir)
    fresh = MyAutoModelWithValueHead.from_pretrained(ckpt, v_head_init_strategy="normal", v_head_initializer_range=0.2, seed=3)
    flat0 = fresh.engine.policy.flat.clone()
    del fresh
    tr = ppo.main(_ppo_args(ckpt, rm_dir, out))
    torch.cuda.synchronize()
    eng = tr.model.engine
    # ---- two steps (five rows, batches of two: the last row is dropped), every stat finite, the game log of the first rows
    assert tr.state.global_step == 2 and len(tr.log_history) == 2 and tr.last_rollout is None
    for h in tr.log_history:
        assert all(torch.isfinite(torch.tensor(v)) for k, v in h.items() if k.startswith(("ppo/", "objective/", "tokens/")))
        assert len(h["game_log"]) == 2 and all("<image>" not in g["query"] and isinstance(g["response"], str) for g in h["game_log"])
        assert 1 <= h["tokens/responses_len_mean"] <= 4
    assert abs(tr.log_history[0]["ppo/mean_scores"] - sum(g["reward"] for g in tr.log_history[0]["game_log"]) / 2) < 1e-6
    # ---- the policy and the head moved, the reference (the frozen copy made at construction) did not
    off, H = eng.layout.offset["v_head.w"], eng.H
    assert flat0.numel() == eng.policy.flat.numel() and not torch.equal(eng.policy.flat[:off], flat0[:off])
    assert not torch.equal(eng.policy.flat[off: off + H], flat0[off: off + H])
    assert torch.equal(tr.ref_model.weights.flat, flat0)
    # ---- kl_coef follows the controller from the logged KL
    c = 0.2
    for h in tr.log_history:
        assert h["objective/kl_coef"] == c
        c *= 1.0 + min(max(h["objective/kl"] / 6.0 - 1.0, -0.2), 0.2) * 2 / 100.0
    assert abs(tr.kl_ctl.value - c) < 1e-12
    # ---- files: a checkpoint per step, the final model with its head, the processor
    for fn in ("checkpoint-1/trainer_state.json", "checkpoint-1/model.safetensors", "checkpoint-1/v_head.bin", "checkpoint-1/optimizer_master.safetensors",
               "checkpoint-2/trainer_state.json", "config.json", "model.safetensors", "v_head.bin", "tokenizer.json"):
        assert os.path.isfile(os.path.join(out, fn)), fn
    final_flat, final_kl, final_perm = eng.policy.flat.clone(), tr.kl_ctl.value, tr._perm_gen.get_state().clone()
    again = MyAutoModelWithValueHead.from_pretrained(out)
    assert torch.equal(again.engine.policy.flat, final_flat)                # what was written reloads to the trained bits, head included
    del again
    # ---- a batch whose scoring raises is skipped: no step for it, the next batch runs
    calls = {"n": 0}
    score = tr.reward_model.score

    def flaky(*a, **k):
        calls["n"] += 1
        if calls["n"] == 1:
            raise RuntimeError("scoring failed")
        return score(*a, **k)
    monkeypatch.setattr(tr.reward_model, "score", flaky)
    tr.config.save_steps = 0
    tr.train()
    assert calls["n"] == 2 and tr.skipped_batches == 1 and tr.state.global_step == 3 and len(tr.log_history) == 3
    del tr
    # ---- resume from the first checkpoint: the second batch alone, to the same bits (greedy sampling, no dropout)
    tr2 = ppo.main(_ppo_args(ckpt, rm_dir, str(tmp_path / "out2"), resume_from_checkpoint=os.path.join(out, "checkpoint-1"), save_steps=0))
    torch.cuda.synchronize()
    assert tr2.state.global_step == 2 and len(tr2.log_history) == 2 and tr2.model.engine.opt_step == 2
    assert tr2.kl_ctl.value == final_kl and torch.equal(tr2._perm_gen.get_state(), final_perm)
    assert torch.equal(tr2.model.engine.policy.flat, final_flat)


def test_value_head_over_a_packed_base_is_refused(gpu, tmp_path):
    """q_lora: a GPTQ checkpoint loads packed, and the value-head model refuses it by name"""
    from tests import gptq_ref
    from vlrlhf.models.Llava import _hf_from_cfg
    from vlrlhf.utils.auto_load import MyAutoModelWithValueHead
    z, cfg, W, W_ref, batch, rows = load_case(CASES[0])
    gptq_ref.write_checkpoint(str(tmp_path), _hf_from_cfg(cfg), W, 32)
    with pytest.raises(NotImplementedError, match="q_lora"):
        MyAutoModelWithValueHead.from_pretrained(str(tmp_path))
