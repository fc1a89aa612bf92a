"""The policy entropy end to end on the MI355X (LLaVA-1.5 and Qwen-VL), on the committed toy fixtures of tests/test_hip_grpo.py and
tests/test_hip_ppo.py: token_logps(return_entropy=True) against the engine's own logits and against the oracle's, the log-probs unmoved;
the GRPO step with the entropy bonus and the high-entropy mask against torch autograd through the oracle (bounds: the constants of
tests/test_hip_grpo.py); the stats keys of both trainers with the options off and on; a 2 x 2 trajectory; checkpoint and resume.
Needs a real MI355X:  pytest -m gpu"""
import functools
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import entropy_ref as ER  # noqa: E402
from tests import grpo_ref as GR  # noqa: E402
from tests import ppo_ref as PR  # noqa: E402
from tests import test_hip_grpo as TG  # noqa: E402
from tests import test_hip_ppo as TP  # noqa: E402
from tests.golden_util import load_case  # noqa: E402
from tests.test_hip_e2e import EMU, cosine, gpu, relmax  # noqa: E402,F401

CASES = TG.CASES
P, G, SCORES = TG.P, TG.G, TG.SCORES
ENT_HP = dict(TG.HP, entropy_coef=1e-3, top_entropy_quantile=0.5)
GRPO_KEYS = {"grpo/loss", "grpo/kl", "grpo/ratio", "grpo/clip_ratio/low", "grpo/clip_ratio/high", "grpo/clip_ratio/region", "grpo/reward_mean",
             "grpo/reward_std", "grpo/frac_reward_zero_std", "grpo/clipped_completions_frac", "tokens/queries_len_mean", "tokens/responses_len_mean",
             "grpo/learning_rate"}
PPO_KEYS = {"objective/kl", "objective/kl_coef", "ppo/loss/policy", "ppo/loss/value", "ppo/loss/total", "ppo/policy/approxkl", "ppo/policy/policykl",
            "ppo/policy/clipfrac", "ppo/policy/advantages_mean", "ppo/policy/ratio", "ppo/returns/mean", "ppo/returns/var", "ppo/val/vpred",
            "ppo/val/error", "ppo/val/clipfrac", "ppo/val/mean", "ppo/val/var", "ppo/mean_scores", "ppo/std_scores", "ppo/mean_non_score_reward",
            "tokens/queries_len_mean", "tokens/responses_len_mean", "ppo/learning_rate"}


def _record(line):
    f = os.environ.get("VLR_ENTROPY_MARGINS")
    print(line)
    if f:
        with open(f, "a") as fh:
            fh.write(line + "\n")


def _lipschitz(logits):
    """sum_v p_v |log p_v + H| per row, fp64: how far a row's entropy moves per unit of (uniformly bounded) logit deviation"""
    lsm = torch.log_softmax(logits.double(), -1)
    p = torch.exp(lsm)
    Hh = -(p * lsm).sum(-1, keepdim=True)
    return (p * (lsm + Hh).abs()).sum(-1), Hh[:, 0]


@functools.lru_cache(maxsize=None)
def oracle_fwd(case):
    z, cfg, W, W_ref, batch, _ = load_case(case)
    with torch.no_grad():
        return ER.oracle_heads(W, cfg, PR.ppo_batch(batch))


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("case", CASES)
def test_entropy_of_the_forward_and_unmoved_logps(gpu, case):
    from vlrlhf.base.model import token_logps
    cfg, W, pb, model, tr = TG.build(case)
    args = (pb["input_ids"].cuda(), pb["attention_mask"].cuda(), pb["labels"].cuda())
    model.eval()
    with torch.no_grad():
        plain = token_logps(model, *args, pixel_values=pb["pixel_values"].cuda()).clone()
        tok, ent = token_logps(model, *args, return_entropy=True, pixel_values=pb["pixel_values"].cuda())
    lp = model._last_lp
    assert ent.dtype == torch.float32 and ent.shape == tok.shape == plain.shape and lp["entropy"] is ent
    assert torch.equal(tok.view(torch.int32), plain.view(torch.int32))                 # switching the entropy on moves no log-prob
    # ---- against the engine's own logits of the same pass: isolates the new code
    V = cfg["vocab"]
    R = lp["R"]                                                # (rows and tgt are allocated for every row of the batch: the first R are filled)
    logits = model.engine.materialize_logits(lp["ctx"]).reshape(-1, V)[lp["rows"][:R].long()]
    ref = ER.forward_reference(lp["hg"], lp["ctx"]["ws"].v["lm_head"], lp["tgt"][:R])
    fails, worst = ER.check_entropy(ent, ref, V)
    assert fails == [], fails
    lip, H_mat = _lipschitz(logits)
    # the materialised logits carry their own accumulation error (<= ez per element): its reach into the entropy is inside b_H as well
    d_own = (ent.double() - H_mat).abs()
    assert bool((d_own <= 2 * ref["b_H"]).all()), float((d_own / ref["b_H"]).max())
    # ---- against the oracle's fp32 logits: the tolerance is the Lipschitz constant times the logit deviation measured here
    o_tok, o_ent, o_logits, o_so = oracle_fwd(case)
    assert lp["seq_off"].tolist() == o_so
    dev = (logits.double().cpu() - o_logits.double()).abs().max(-1).values            # per row
    lip_o, _ = _lipschitz(o_logits)
    tol = lip_o * dev * (1 + 4 * dev) + dev ** 2 * (2 + math.log(V)) + ref["b_H"].cpu()
    d = (ent.double().cpu() - o_ent.double()).abs()
    _record(f"{case:16s} entropy: kernel err/bound {worst:.3f}; |H - H(engine logits)| {float(d_own.max()):.3e}; logit deviation engine vs oracle "
            f"{float(dev.max()):.3e}; |H - oracle| {float(d.max()):.3e} (worst / tolerance {float((d / tol).max()):.3f}); mean H {float(o_ent.mean()):.4f}")
    assert bool((d <= tol).all())
    # ---- the value-head wrapper's switch (PPO's statistic): the same rows, the same bits
    cfg, W, pb, vmodel, _ = TP.build(case)
    vmodel.eval()
    with torch.no_grad():
        t3 = vmodel(*args, pixel_values=pb["pixel_values"].cuda())
        t4 = vmodel(*args, return_entropy=True, pixel_values=pb["pixel_values"].cuda())
    assert len(t3) == 3 and len(t4) == 4 and torch.equal(t3[0], t4[0]) and torch.equal(t3[2], t4[2])
    assert torch.equal(t4[3].view(torch.int32), ent.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ 2
def test_high_entropy_mask_keeps_ties(gpu):
    """q = 0.5 on entropies with ties: what torch.quantile (linear interpolation) and >= keep, the threshold's own ties included"""
    from vlrlhf.base.trainer import GRPOConfig, high_entropy_mask
    h = torch.tensor([0.5, 2.0, 1.0, 1.0, 1.0, 3.0, 0.25, 1.0])
    keep = high_entropy_mask(h.cuda(), 0.5)
    assert keep.dtype == torch.uint8 and keep.is_cuda
    assert keep.cpu().bool().tolist() == (h >= torch.quantile(h, 0.5)).tolist() == [False, True, True, True, True, True, False, True]
    h2 = torch.tensor([0.1, 0.2, 0.3, 0.4])                    # the threshold falls between two tokens
    assert high_entropy_mask(h2.cuda(), 0.5).cpu().tolist() == [0, 0, 1, 1]
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="top_entropy_quantile"):
            GRPOConfig(top_entropy_quantile=bad)


# ------------------------------------------------------------------------------------------------------------ 3
@functools.lru_cache(maxsize=None)
def oracle_step(case, coef, q, beta, zero_adv):
    z, cfg, W, W_ref, batch, _ = load_case(case)
    _, _, pb4 = TG._group_rows(PR.ppo_batch(batch))
    hp = dict(TG.HP, entropy_coef=coef, top_entropy_quantile=q, beta=beta)
    scores = torch.tensor((1.0, 1.0, 0.5, 0.5) if zero_adv else SCORES)
    return ER.step_grads(W, W_ref, cfg, pb4, scores, P, G, hp, [list(range(P * G))], TP._grad_names(cfg), 1.0)


@pytest.mark.parametrize("case", CASES)
def test_step_with_bonus_and_mask_matches_oracle(gpu, case):
    """entropy_coef > 0 and top_entropy_quantile = 0.5, the whole batch in one minibatch: loss, every stat and the gradient against autograd
    through the oracle, within the bounds tests/test_hip_grpo.py holds the plain step to"""
    cfg, W, pb, model, tr = TG.build(case, entropy_coef=ENT_HP["entropy_coef"], top_entropy_quantile=0.5, log_entropy=True)
    exp = oracle_step(case, ENT_HP["entropy_coef"], 0.5, TG.HP["beta"], False)
    qs, rs, _ = TG._group_rows(pb)
    stats = tr.step(qs, rs, list(SCORES), pixel_values=pb["pixel_values"])
    torch.cuda.synchronize()
    ro = tr.last_rollout
    ent, keep = ro["minibatch_entropy"][0]
    want = exp["stats"][0]
    R = ent.numel()
    # the mask: the HIP path keeps what torch.quantile + >= keep on ITS entropies, and those are the tokens the oracle keeps
    assert keep.cpu().bool().tolist() == (ent.cpu() >= torch.quantile(ent.cpu(), 0.5)).tolist()
    thr = float(torch.quantile(exp["entropy"][0], 0.5))
    _record(f"{case:16s} mask: {int(keep.sum())} of {R} kept; the oracle's closest entropy to its threshold {float((exp['entropy'][0] - thr).abs().min()):.3e}; "
            f"max |H - oracle| {float((ent.cpu() - exp['entropy'][0]).abs().max()):.3e}")
    assert keep.cpu().bool().tolist() == exp["keep"][0].tolist()
    assert set(stats) == GRPO_KEYS | {"grpo/entropy", "grpo/entropy_kept_frac"} and all(math.isfinite(v) for v in stats.values())
    d_loss, d_kl, d_ent = abs(stats["grpo/loss"] - want["loss"]), abs(stats["grpo/kl"] - want["kl"]), abs(stats["grpo/entropy"] - want["entropy"])
    _record(f"{case:16s} step with bonus and mask: loss {d_loss:.3e} (hip {stats['grpo/loss']:.6f} oracle {want['loss']:.6f})  kl {d_kl:.3e}  "
            f"entropy {d_ent:.3e} (oracle {want['entropy']:.5f})  kept {stats['grpo/entropy_kept_frac']:.4f}")
    assert d_loss <= TG.TOL_LOSS[case] and d_kl <= TG.TOL_KL[case]
    assert abs(stats["grpo/entropy_kept_frac"] - want["kept_frac"]) <= 4 * ER.U and abs(stats["grpo/entropy_kept_frac"] - int(keep.sum()) / R) <= 4 * ER.U
    assert d_ent <= float((ent.cpu() - exp["entropy"][0]).abs().max()) + 1e-6             # a mean moves no further than its terms
    assert stats["grpo/ratio"] == 1.0 and stats["grpo/clip_ratio/region"] == 0.0
    ms = ro["minibatch_stats"][0].tolist()
    assert len(ms) == 10 and (stats["grpo/loss"], stats["grpo/kl"], stats["grpo/entropy"], stats["grpo/entropy_kept_frac"]) == (ms[0], ms[1], ms[8], ms[9])
    named = dict(model.named_parameters())
    for n in TP._grad_names(cfg):
        cs, rm = cosine(named[n].grad, exp["grads"][n]), relmax(named[n].grad, exp["grads"][n])
        print(f"[entropy grads] {case} {n}: cosine {cs:.5f} relmax {rm:.3e}")
        assert cs > TP.GRAD_COS and rm < TP.GRAD_RELMAX, (n, cs, rm)


@pytest.mark.parametrize("case", CASES)
def test_gradient_of_the_bonus_alone_matches_oracle(gpu, case):
    """equal scores inside every group (all advantages exactly 0) and beta = 0: the loss is -entropy_coef x the mean entropy and the whole
    gradient comes through the entropy term of the lm-head backward"""
    cfg, W, pb, model, tr = TG.build(case, entropy_coef=1.0, beta=0.0)
    exp = oracle_step(case, 1.0, 1.0, 0.0, True)
    qs, rs, _ = TG._group_rows(pb)
    stats = tr.step(qs, rs, [1.0, 1.0, 0.5, 0.5], pixel_values=pb["pixel_values"])
    torch.cuda.synchronize()
    assert set(stats) == GRPO_KEYS                             # the bonus alone adds no key
    assert bool((tr.last_rollout["advantages"] == 0).all()) and stats["grpo/loss"] < 0
    ent = tr.last_rollout["minibatch_entropy"][0][0].cpu()
    d = abs(stats["grpo/loss"] - exp["stats"][0]["loss"])
    _record(f"{case:16s} bonus alone: loss hip {stats['grpo/loss']:.6f} oracle {exp['stats'][0]['loss']:.6f} |diff| {d:.3e}")
    assert d <= float((ent - exp["entropy"][0]).abs().max()) + 1e-6
    named = dict(model.named_parameters())
    for n in TP._grad_names(cfg):
        cs, rm = cosine(named[n].grad, exp["grads"][n]), relmax(named[n].grad, exp["grads"][n])
        print(f"[entropy bonus grads] {case} {n}: cosine {cs:.5f} relmax {rm:.3e}")
        assert cs > TP.GRAD_COS and rm < TP.GRAD_RELMAX, (n, cs, rm)


# ------------------------------------------------------------------------------------------------------------ 4
def test_stats_keys_with_the_options_off_and_on(gpu):
    case = CASES[0]
    cfg, W, pb, model, tr = TG.build(case)
    qs, rs, _ = TG._group_rows(pb)
    off = tr.step(qs, rs, list(SCORES), pixel_values=pb["pixel_values"])
    assert set(off) == GRPO_KEYS and "minibatch_entropy" not in tr.last_rollout and tr.last_rollout["minibatch_stats"][0].numel() == 8
    cfg, W, pb, model2, tr2 = TG.build(case, log_entropy=True)
    on = tr2.step(qs, rs, list(SCORES), pixel_values=pb["pixel_values"])
    assert set(on) == GRPO_KEYS | {"grpo/entropy"} and all(math.isfinite(v) for v in on.values())
    # logging moves nothing: the same loss bits and the same weights after the step
    assert all(on[k] == off[k] for k in GRPO_KEYS) and torch.equal(model.engine.policy.flat, model2.engine.policy.flat)
    assert 0.0 < on["grpo/entropy"] <= math.log(cfg["vocab"])


@pytest.mark.parametrize("case", CASES)
def test_ppo_entropy_stats(gpu, case):
    from vlrlhf.base.trainer import sequence_neg_logp_mean
    cfg, W, pb, model, tr = TP.build(case)
    qs, rs = TP._split(pb)
    off = tr.step(qs, rs, list(TP.SCORES), pixel_values=pb["pixel_values"])
    assert set(off) == PPO_KEYS
    cfg, W, pb, model2, tr2 = TP.build(case, log_entropy=True)
    # the logit deviation between the engine and the oracle at the step's first weights, measured on a no-grad pass before the step
    o_tok, o_ent, o_logits, _ = oracle_fwd(case)
    with torch.no_grad():
        model2(pb["input_ids"].cuda(), pb["attention_mask"].cuda(), pb["labels"].cuda(), pixel_values=pb["pixel_values"].cuda())
    lp = model2._last_lp
    V = cfg["vocab"]
    logits = model2.engine.materialize_logits(lp["ctx"]).reshape(-1, V)[lp["rows"][:lp["R"]].long()]
    dev = (logits.double().cpu() - o_logits.double()).abs().max(-1).values
    b_H = ER.forward_reference(lp["hg"], lp["ctx"]["ws"].v["lm_head"], lp["tgt"][:lp["R"]])["b_H"].cpu()
    on = tr2.step(qs, rs, list(TP.SCORES), pixel_values=pb["pixel_values"])
    torch.cuda.synchronize()
    assert set(on) == PPO_KEYS | {"ppo/policy/entropy", "objective/entropy"} and all(math.isfinite(v) for v in on.values())
    assert all(on[k] == off[k] for k in PPO_KEYS) and torch.equal(model.engine.policy.flat, model2.engine.policy.flat)
    ro = tr2.last_rollout
    x, so = ro["old_logp"].double().cpu(), ro["seq_off"]
    assert on["objective/entropy"] == sum(-float(x[so[s]:so[s + 1]].sum()) for s in range(len(so) - 1)) / (len(so) - 1) \
        == sequence_neg_logp_mean(ro["old_logp"], so)
    # trl's masked_mean(entropy_from_logits(logits), mask) on the minibatch (the whole batch, at the step's first weights)
    d = abs(on["ppo/policy/entropy"] - float(o_ent.double().mean()))
    lip, _ = _lipschitz(o_logits)
    # a mean moves no further than its terms: per row the Lipschitz constant x the measured logit deviation + the kernel's own bound
    tol = float((lip * dev * (1 + 4 * dev) + dev ** 2 * (2 + math.log(V)) + b_H).mean()) + 4 * ER.U * math.log(V)
    _record(f"{case:16s} ppo/policy/entropy hip {on['ppo/policy/entropy']:.5f} oracle {float(o_ent.mean()):.5f} |diff| {d:.3e} (tolerance {tol:.3e}); "
            f"objective/entropy {on['objective/entropy']:.5f}")
    assert d <= tol


# ------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("case", CASES)
def test_trajectory_with_the_options_on_tracks_the_oracle_loop(gpu, case):
    """2 steps x 2 iterations x 2 minibatches of one group with the bonus and the mask, against the oracle loop of tests/entropy_ref.py,
    within the trajectory bounds of tests/test_hip_grpo.py"""
    lr = 2e-5
    cfg, W, pb, model, tr = TG.build(case, mini_batch_size=G, num_iterations=2, learning_rate=lr, log_entropy=True,
                                     entropy_coef=ENT_HP["entropy_coef"], top_entropy_quantile=0.5)
    qs, rs, pb4 = TG._group_rows(pb)
    hip, kept = [], []
    for _ in range(2):
        tr.step(qs, rs, list(SCORES), pixel_values=pb["pixel_values"])
        ms = tr.last_rollout["minibatch_stats"]
        assert len(ms) == 4
        hip += [float(st[0]) for st in ms]
        kept += [float(st[9]) for st in ms]
    torch.cuda.synchronize()
    assert model.engine.opt_step == 8
    z, _, _, W_ref, _, _ = load_case(case)
    emu = (EMU | {"vit"}) if "visual" in cfg else EMU
    o_stats = ER.train_steps(W, W_ref, cfg, pb4, torch.tensor(SCORES), P, G, ENT_HP, 2, 2, G, lr, emulate=emu)
    ora = [st["loss"] for st in o_stats]
    worst = max(abs(h - r) for h, r in zip(hip, ora))
    _record(f"{case:16s} entropy trajectory hip    " + " ".join(f"{x:.6f}" for x in hip))
    _record(f"{case:16s} entropy trajectory oracle " + " ".join(f"{x:.6f}" for x in ora))
    _record(f"{case:16s} entropy trajectory worst |hip - oracle| over 8 minibatches {worst:.3e}; kept fractions hip {kept} oracle "
            f"{[st['kept_frac'] for st in o_stats]}")
    assert len(hip) == len(ora) == 8 and worst <= TG.TOL_TRAJECTORY[case], (hip, ora)
    assert all(abs(a - st["kept_frac"]) <= 4 * ER.U for a, st in zip(kept, o_stats))      # the same number of tokens kept in every minibatch


# ------------------------------------------------------------------------------------------------------------ 6
def test_checkpoint_and_resume_with_the_options_on(gpu, tmp_path):
    """vlrlhf.grpo.main with the three options: a run resumed from the first checkpoint lands on the bits of the uninterrupted one"""
    from tests.golden_util import write_tiny_checkpoint
    from vlrlhf import grpo
    ckpt, out = str(tmp_path / "ckpt"), str(tmp_path / "out")
    write_tiny_checkpoint(ckpt)
    opts = dict(log_entropy=True, top_entropy_quantile=0.5, entropy_coef=0.01)
    tr = grpo.main(TG._grpo_args(ckpt, out, **opts), reward_fn=TG._reward)
    torch.cuda.synchronize()
    assert tr.state.global_step == 2 and tr.model.engine.opt_step == 8
    for h in tr.log_history:
        assert math.isfinite(h["grpo/entropy"]) and 0.0 < h["grpo/entropy_kept_frac"] <= 1.0
    final_flat, final_gen = tr.model.engine.policy.flat.clone(), tr._sample_gen.get_state().clone()
    del tr
    tr2 = grpo.main(TG._grpo_args(ckpt, str(tmp_path / "out2"), resume_from_checkpoint=os.path.join(out, "checkpoint-1"), save_steps=0, **opts),
                    reward_fn=TG._reward)
    torch.cuda.synchronize()
    assert tr2.state.global_step == 2 and tr2.model.engine.opt_step == 8
    assert torch.equal(tr2._sample_gen.get_state(), final_gen) and torch.equal(tr2.model.engine.policy.flat, final_flat)
