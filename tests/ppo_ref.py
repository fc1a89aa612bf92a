"""Checker side of the PPO tests: the PPO step of include/vlr.h ("PPO") restated in plain torch on the CPU.  Everything that replays a
kernel runs in fp64 on the kernel's own fp32 inputs; the loss is ONE torch expression, so its gradients are torch autograd's, ties
included (torch.clamp passes the gradient on its closed interval, torch.max halves a tie).  All per-token tensors are compact [R] over
the response rows, seq_off [n + 1] delimits the sequences."""
import math

import torch

KL_MODES = {"kl": 0, "abs": 1, "mse": 2}


def kl_penalty(old_logp, ref_logp, mode):
    d = old_logp - ref_logp
    if mode == "kl":
        return d
    if mode == "abs":
        return d.abs()
    if mode == "mse":
        return 0.5 * d * d
    if mode == "full":
        raise NotImplementedError("kl_penalty='full' needs the [R][V] logits of both models")
    raise ValueError(f"unknown kl_penalty {mode!r}")


def masked_whiten(x, shift_mean=True):
    """(x - mean) * rsqrt(var + 1e-8) over ALL tokens, var = the biased variance * R / (R - 1); shift_mean=False adds the mean back"""
    R = x.numel()
    if R < 2:
        raise ValueError(f"masked_whiten needs at least 2 tokens, got {R}")
    mean = x.mean()
    var = ((x - mean) ** 2).mean() * (R / (R - 1))
    y = (x - mean) * torch.rsqrt(var + 1e-8)
    return y if shift_mean else y + mean


def rewards(old_logp, ref_logp, seq_off, scores, kl_coef, mode="kl"):
    """-> (rewards [R], non-score rewards [R], kl [R]): -kl_coef kl_t, + score on the last token of each sequence"""
    kl = kl_penalty(old_logp, ref_logp, mode)
    nsr = -kl_coef * kl
    r = nsr.clone()
    for s in range(len(seq_off) - 1):
        if seq_off[s + 1] > seq_off[s]:
            r[seq_off[s + 1] - 1] += scores[s]
    return r, nsr, kl


def gae(r, values, seq_off, gamma, lam):
    """per sequence, backwards: delta_t = r_t + gamma V_{t+1} - V_t (V past the end = 0), A_t = delta_t + gamma lam A_{t+1} -> (A, A + V)"""
    adv = torch.zeros_like(r)
    for s in range(len(seq_off) - 1):
        a, vn = 0.0, 0.0
        for t in range(int(seq_off[s + 1]) - 1, int(seq_off[s]) - 1, -1):
            delta = r[t] + gamma * vn - values[t]
            a = delta + gamma * lam * a
            adv[t] = a
            vn = values[t]
    return adv, adv + values


def advantages(old_logp, ref_logp, values, seq_off, scores, kl_coef, mode, gamma, lam, whiten_rewards):
    """vlr_ppo_advantages in fp64 -> dict(advantages, returns, kl_sums [n], stats [4], rewards, raw_advantages)"""
    old_logp, ref_logp, values, scores = (t.double() for t in (old_logp, ref_logp, values, scores))
    seq_off = [int(x) for x in seq_off]
    r, nsr, kl = rewards(old_logp, ref_logp, seq_off, scores, kl_coef, mode)
    if whiten_rewards:
        r = masked_whiten(r, shift_mean=False)
    raw, ret = gae(r, values, seq_off, gamma, lam)
    R = raw.numel()
    kl_sums = torch.stack([kl[seq_off[s]:seq_off[s + 1]].sum() for s in range(len(seq_off) - 1)])
    mean = raw.mean()
    var = ((raw - mean) ** 2).mean() * (R / (R - 1))
    stats = torch.stack([kl_sums.mean(), nsr.mean(), mean, var])
    return dict(advantages=masked_whiten(raw), returns=ret, kl_sums=kl_sums, stats=stats, rewards=r, raw_advantages=raw)


def masked_var(x):
    R = x.numel()
    return ((x - x.mean()) ** 2).mean() * (R / (R - 1))


STAT_NAMES = ("loss", "pg", "vf", "approxkl", "policykl", "pg_clipfrac", "vf_clipfrac", "ratio", "returns_mean", "returns_var", "vpred_mean",
              "vpred_var", "error", "advantages_mean", "values_mean", "values_var", "skipped")


def loss(logp, vpred, old_logp, old_values, adv, ret, cr, crv, vf_coef, ratio_threshold, upstream=1.0):
    """vlr_ppo_loss as ONE differentiable torch expression in the dtype of `logp` (fp64 to replay the kernel, fp32 inside the end-to-end
    oracle) -> (loss tensor with its graph, stats dict of floats in the order of STAT_NAMES).  loss.backward() * upstream are the
    gradients the kernel returns."""
    ratio = torch.exp(logp - old_logp)
    pg1 = -adv * ratio
    pg2 = -adv * torch.clamp(ratio, 1.0 - cr, 1.0 + cr)
    pg = torch.max(pg1, pg2).mean()
    vclip = torch.clamp(vpred, old_values - crv, old_values + crv)
    l1, l2 = (vpred - ret) ** 2, (vclip - ret) ** 2
    vf = 0.5 * torch.max(l1, l2).mean()
    total = pg + vf_coef * vf
    skipped = bool(ratio.mean() > ratio_threshold)
    if skipped:
        pg, vf, total = pg * 0.0, vf * 0.0, total * 0.0
    stats = dict(loss=total, pg=pg, vf=vf, approxkl=0.5 * ((logp - old_logp) ** 2).mean(), policykl=(old_logp - logp).mean(),
                 pg_clipfrac=(pg2 > pg1).double().mean(), vf_clipfrac=(l2 > l1).double().mean(), ratio=ratio.mean(), returns_mean=ret.mean(),
                 returns_var=masked_var(ret), vpred_mean=vpred.mean(), vpred_var=masked_var(vpred), error=l1.mean(), advantages_mean=adv.mean(),
                 values_mean=old_values.mean(), values_var=masked_var(old_values), skipped=torch.tensor(float(skipped)))
    return total * upstream, {k: float(v.detach()) for k, v in stats.items()}


def loss_and_grads(logp, vpred, old_logp, old_values, adv, ret, cr, crv, vf_coef, ratio_threshold, upstream=1.0):
    """fp64 replay of vlr_ppo_loss -> (stats dict, dlogp [R], dvpred [R])"""
    lp, vp = logp.double().clone().requires_grad_(True), vpred.double().clone().requires_grad_(True)
    total, stats = loss(lp, vp, old_logp.double(), old_values.double(), adv.double(), ret.double(), cr, crv, vf_coef, ratio_threshold, upstream)
    total.backward()
    return stats, lp.grad, vp.grad


def v_head_bwd(hg, w, g, dhg, dw_old=None, db_old=None):
    """fp64 replay of vlr_v_head_bwd -> (dhg + g w [R][H], dw [H], db), the old head gradients added when given"""
    hg, w, g, dhg = hg.double(), w.double(), g.double(), dhg.double()
    dw, db = g @ hg, g.sum()
    if dw_old is not None:
        dw, db = dw + dw_old.double(), db + db_old.double()
    return dhg + g[:, None] * w[None, :], dw, db


class AdaptiveKLController:
    """trl's controller: e = clip(kl / target - 1, -0.2, 0.2); kl_coef *= 1 + e * n_steps / horizon"""

    def __init__(self, init_kl_coef, target, horizon):
        self.value, self.target, self.horizon = init_kl_coef, target, horizon

    def update(self, current, n_steps):
        e = min(max(current / self.target - 1.0, -0.2), 0.2)
        self.value *= 1.0 + e * n_steps / self.horizon


class FixedKLController:
    def __init__(self, kl_coef):
        self.value = kl_coef

    def update(self, current, n_steps):
        pass


# ------------------------------------------------------------------------------------------------------------ the policy through the oracles
V_HEAD_BIAS = 0.125


def v_head(H, seed=11):
    """the value head of the tests: w ~ U(-1, 1) / sqrt(H) from a seeded host generator, bias 0.125 -> (w [H] fp32, b [1] fp32)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(H, generator=g) * 2 - 1) / math.sqrt(H), torch.tensor([V_HEAD_BIAS])


def ppo_batch(batch, side="chosen"):
    """one side of a DPO fixture batch as PPO sees it: [query ; response] right-padded, labels -100 except on the response tokens"""
    return dict(input_ids=batch[f"{side}_input_ids"], attention_mask=batch[f"{side}_attention_mask"], labels=batch[f"{side}_labels"],
                pixel_values=batch["img_input_dict"]["pixel_values"])


def policy_heads(W, cfg, pb, w, b, emulate=False, lora=None):
    """(token log-probs [R], values [R], seq_off [n + 1]) of the family's oracle forward on the response rows: the positions whose logits
    predict a token with label != -100, sequence after sequence; the values read the same positions (trl: values[:, :-1]).  `lora`: the
    oracle's adapter dict (random_lora), its tensors under lora["W"]"""
    from oracle import llava_dpo_oracle as O
    from oracle import qwenvl_oracle as Q
    px = pb["pixel_values"].float()
    if cfg.get("family") == "qwen_vl" or "visual" in cfg:
        hidden = Q.qwenvl_forward(W, cfg, pb["input_ids"], pb["attention_mask"], px, emulate_bf16=emulate, return_hidden=True, dedupe_images=False,
                                  lora=lora)[0]
        labels, key = pb["labels"], "lm_head.weight"
    else:
        hidden, labels, _ = O.llava_forward(W, cfg, pb["input_ids"], pb["attention_mask"], pb["labels"], px, emulate_bf16=emulate,
                                            dedupe_images=False, return_hidden=True, lora=lora)
        key = "language_model.lm_head.weight"
    sel = labels[:, 1:] != -100
    h = hidden[:, :-1][sel]                                               # [R, H], row-major over (sequence, position)
    logits = O.lm_logits(h, W, emulate, key=key)
    tok = torch.log_softmax(logits.float(), -1).gather(-1, labels[:, 1:][sel].unsqueeze(-1)).squeeze(-1)
    values = h.float() @ w.float() + b.float()
    seq_off = [0] + torch.cumsum(sel.sum(-1), 0).tolist()
    return tok, values, seq_off


def minibatch_loss_and_grads(W, W_ref, cfg, pb, w, b, scores, hp, names, emulate=False):
    """the first minibatch of a PPO step through the oracle, in fp32: rollout (old log-probs / values of the policy, log-probs of the
    reference) under no-grad, advantages and returns from them (fp64 replay, rounded to fp32), then the loss with torch autograd.
    -> dict(tok, values, ref, advantages, returns, kl_sums, adv_stats, stats, grads {name: grad} incl. the two v_head.summary.* keys)"""
    with torch.no_grad():
        old_logp, old_values, seq_off = policy_heads(W, cfg, pb, w, b, emulate)
        ref_logp, _, _ = policy_heads(W_ref, cfg, pb, w, b, emulate)
    adv = advantages(old_logp, ref_logp, old_values, seq_off, scores, hp["kl_coef"], hp["kl_penalty"], hp["gamma"], hp["lam"], hp["whiten_rewards"])
    leaves = {k: W[k].clone().requires_grad_(True) for k in names}
    wl, bl = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    Wl = dict(W)
    Wl.update(leaves)
    logp, vpred, _ = policy_heads(Wl, cfg, pb, wl, bl, emulate)
    total, stats = loss(logp, vpred, old_logp, old_values, adv["advantages"].float(), adv["returns"].float(), hp["cliprange"],
                        hp["cliprange_value"], hp["vf_coef"], hp["ratio_threshold"])
    total.backward()
    g = {k: v.grad for k, v in leaves.items()}
    g["v_head.summary.weight"], g["v_head.summary.bias"] = wl.grad, bl.grad
    return dict(tok=old_logp, values=old_values, ref=ref_logp, seq_off=seq_off, advantages=adv["advantages"], returns=adv["returns"],
                kl_sums=adv["kl_sums"], adv_stats=adv["stats"], stats=stats, grads=g)


def _rows(pb, cfg, rows):
    """the batch rows `rows` (in that order) at the batch's padded width, with the images those rows name"""
    ids = pb["input_ids"]
    tok = cfg["image_start_id"] if "visual" in cfg else cfg["image_token"]
    off = [0] + torch.cumsum((ids == tok).sum(-1), 0).tolist()
    img = [j for r in rows for j in range(off[r], off[r + 1])]
    return dict(input_ids=ids[rows], attention_mask=pb["attention_mask"][rows], labels=pb["labels"][rows], pixel_values=pb["pixel_values"][img])


def train_steps(W, W_ref, cfg, pb, w, b, scores, hp, steps, ppo_epochs, mini_batch_size, lr, seed, emulate=False, lora=None):
    """`steps` PPO steps of a full fine-tune the way the HIP path stores things: fp32 master weights made from the bf16 weights (head included), every pass on their
    bf16 rounding, one Adam step (weight decay 0, no clipping) per minibatch, a fresh permutation per epoch from a generator seeded by
    `seed`, the adaptive KL controller between steps.  With `lora` (the oracle's adapter dict) only the adapters and the head train, the base is
    frozen and the reference is the adapter-free pass over it (W_ref is not read).  -> (per-minibatch stats dicts, objective/kl per step, kl_coef after each step)"""
    from oracle import llava_dpo_oracle as O
    # what a full fine-tune trains on the HIP path: everything but the vision tower - of Qwen-VL's, the resampler (attn_pool, without its
    # fixed pos_embed) stays trainable (reference models/QwenVL/__init__.py freeze_vision_tower)
    ap = "transformer.visual.attn_pool."
    names = [n for n in O.trainable_names(W) if not n.startswith("transformer.visual.") or (n.startswith(ap) and n != ap + "pos_embed")]
    # the engine's master copy is made FROM its bf16 weights (init_optimizer), so every master starts on the bf16 grid: from there an Adam
    # update below half a grid step changes no weight, where a master started off the grid would flip some
    master = {k: v.bfloat16().float() for k, v in W.items()}
    if lora is not None:
        names = list(lora["W"])
        master.update({k: v.bfloat16().float() for k, v in lora["W"].items()})
    with_lora = (lambda Wd: dict(lora, W={k: Wd[k] for k in lora["W"]})) if lora is not None else (lambda Wd: None)      # noqa: E731
    master["v_head.summary.weight"], master["v_head.summary.bias"] = w.bfloat16().float(), b.bfloat16().float()
    state, losses, kls, coefs = {}, [], [], []
    gen = torch.Generator().manual_seed(seed)
    ctl = AdaptiveKLController(hp["kl_coef"], hp["target"], hp["horizon"])
    n = pb["input_ids"].shape[0]
    rnd = lambda: {k: v.bfloat16().float() for k, v in master.items()}      # noqa: E731
    for _ in range(steps):
        Wp = rnd()
        with torch.no_grad():
            old_logp, old_values, seq_off = policy_heads(Wp, cfg, pb, Wp["v_head.summary.weight"], Wp["v_head.summary.bias"], emulate, with_lora(Wp))
            ref_logp, _, _ = policy_heads(W_ref if lora is None else Wp, cfg, pb, w, b, emulate)
        adv = advantages(old_logp, ref_logp, old_values, seq_off, scores, ctl.value, hp["kl_penalty"], hp["gamma"], hp["lam"], hp["whiten_rewards"])
        A, ret = adv["advantages"].float(), adv["returns"].float()
        for _ in range(ppo_epochs):
            perm = torch.randperm(n, generator=gen).tolist()
            for m0 in range(0, n, mini_batch_size):
                rows = perm[m0:m0 + mini_batch_size]
                tok = torch.tensor([t for r in rows for t in range(seq_off[r], seq_off[r + 1])], dtype=torch.long)
                leaves = {k: Wp[k].clone().requires_grad_(True) for k in names + ["v_head.summary.weight", "v_head.summary.bias"]}
                Wl = dict(Wp)
                Wl.update(leaves)
                logp, vpred, _ = policy_heads(Wl, cfg, _rows(pb, cfg, rows), leaves["v_head.summary.weight"], leaves["v_head.summary.bias"], emulate,
                                                  with_lora(Wl))
                total, st = loss(logp, vpred, old_logp[tok], old_values[tok], A[tok], ret[tok], hp["cliprange"], hp["cliprange_value"],
                                 hp["vf_coef"], hp["ratio_threshold"])
                total.backward()
                grads = {k: v.grad for k, v in leaves.items() if v.grad is not None}
                with torch.no_grad():
                    O.adamw_step(master, grads, state, lr, 0.9, 0.999, 1e-8, 0.0)
                Wp = rnd()
                losses.append(st)
        kls.append(float(adv["stats"][0]))
        ctl.update(kls[-1], n)
        coefs.append(ctl.value)
    return losses, kls, coefs


def accumulated_grads(W, W_ref, cfg, pb, w, b, scores, hp, minibatches, names, upstream):
    """the gradient one backward batch leaves behind: every minibatch (a list of rows) at the SAME weights, its loss scaled by `upstream`,
    the gradients added - in fp32 through the oracle.  -> {name: grad} incl. the two v_head.summary.* keys"""
    with torch.no_grad():
        old_logp, old_values, seq_off = policy_heads(W, cfg, pb, w, b)
        ref_logp, _, _ = policy_heads(W_ref, cfg, pb, w, b)
    adv = advantages(old_logp, ref_logp, old_values, seq_off, scores, hp["kl_coef"], hp["kl_penalty"], hp["gamma"], hp["lam"], hp["whiten_rewards"])
    A, ret = adv["advantages"].float(), adv["returns"].float()
    leaves = {k: W[k].clone().requires_grad_(True) for k in names}
    wl, bl = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    Wl = dict(W)
    Wl.update(leaves)
    for rows in minibatches:
        tok = torch.tensor([t for r in rows for t in range(seq_off[r], seq_off[r + 1])], dtype=torch.long)
        logp, vpred, _ = policy_heads(Wl, cfg, _rows(pb, cfg, rows), wl, bl)
        total, _ = loss(logp, vpred, old_logp[tok], old_values[tok], A[tok], ret[tok], hp["cliprange"], hp["cliprange_value"], hp["vf_coef"],
                        hp["ratio_threshold"], upstream)
        total.backward()
    g = {k: v.grad for k, v in leaves.items()}
    g["v_head.summary.weight"], g["v_head.summary.bias"] = wl.grad, bl.grad
    return g
