"""Checker side of the GRPO tests: vlr_grpo_advantages and vlr_grpo_loss of include/vlr.h ("GRPO") restated in plain torch on the CPU.
Everything that replays a kernel runs in fp64 on the kernel's own fp32 inputs; the loss is ONE torch expression, written as the header
writes it, so its gradient is torch autograd's, ties included (torch.clamp passes the gradient on its closed interval, the binary
torch.min halves a tie).  The per-token tensors are compact [R] over the response rows, seq_off [n + 1] delimits the sequences.

check_advantages / check_loss are the ONE comparison the GPU tests use: a kernel's outputs against the fp64 replay, within bounds derived
from the fp32 unit roundoff u = 2^-24, the number of terms a sum folds, the magnitude of the terms and expf's stated 2 ulp - never from a
kernel's output.  tests/test_grpo_checker_host.py plants faults and sees each of them flagged."""
import math

import torch

U = 2.0 ** -24
LOSS_TYPES = {"grpo": 0, "bnpo": 1, "dr_grpo": 2}
ADV_STAT_NAMES = ("reward_mean", "reward_std", "frac_reward_zero_std")
STAT_NAMES = ("loss", "kl", "clip_low", "clip_high", "clip_region", "ratio", "len_mean")
BRANCHES = ("inside", "clipped_low", "clipped_high", "outside_unclipped", "zero_advantage")


# ------------------------------------------------------------------------------------------------------------ the arithmetic
def advantages(scores, P, G, scale_rewards=True):
    """vlr_grpo_advantages in the dtype of `scores` -> (A [P * G], stats [3]: mean of all scores, mean over the groups of the unbiased
    std, fraction of groups whose std is 0)"""
    s = scores.reshape(P, G)
    mean = s.mean(1, keepdim=True)
    std = s.std(1, unbiased=True, keepdim=True)
    A = (s - mean) / (std + 1e-4) if scale_rewards else s - mean
    stats = torch.stack([s.mean(), std.mean(), (std == 0).to(s.dtype).mean()])
    return A.reshape(-1), stats


def _lens(seq_off):
    so = [int(x) for x in seq_off]
    return so, [so[i + 1] - so[i] for i in range(len(so) - 1)]


def loss(logp, old_logp, ref_logp, adv_seq, seq_off, eps_low, eps_high, beta, loss_type, max_completion_length=0, upstream=1.0):
    """vlr_grpo_loss as ONE differentiable torch expression in the dtype of `logp` (fp64 to replay the kernel, fp32 inside the end-to-end
    oracle) -> (loss * upstream with its graph, stats dict of floats under STAT_NAMES).  old_logp None: logp itself, detached.
    loss_type: a name of LOSS_TYPES or its number."""
    lt = LOSS_TYPES.get(loss_type, loss_type)
    so, lens = _lens(seq_off)
    n, R = len(lens), logp.numel()
    old = logp.detach() if old_logp is None else old_logp
    A = torch.repeat_interleave(adv_seq.to(logp.dtype), torch.tensor(lens))
    r = torch.exp(logp - old)
    tok = -torch.min(r * A, torch.clamp(r, 1.0 - eps_low, 1.0 + eps_high) * A)
    kl = torch.zeros_like(tok)
    if beta != 0:
        d = ref_logp - logp
        kl = torch.exp(d) - d - 1.0
        tok = tok + beta * kl
    if lt == 0:
        total = sum(tok[so[s]:so[s + 1]].sum() / lens[s] for s in range(n)) / n
    elif lt == 1:
        total = tok.sum() / R
    elif lt == 2:
        total = tok.sum() / (n * max_completion_length)
    else:
        raise ValueError(f"unknown loss_type {loss_type!r}")
    low = ((r < 1.0 - eps_low) & (A < 0)).to(logp.dtype).mean()
    high = ((r > 1.0 + eps_high) & (A > 0)).to(logp.dtype).mean()
    stats = dict(loss=total, kl=kl.mean(), clip_low=low, clip_high=high, clip_region=low + high, ratio=r.mean(), len_mean=torch.tensor(R / n))
    return total * upstream, {k: float(v.detach()) for k, v in stats.items()}


def loss_and_grad(logp, old_logp, ref_logp, adv_seq, seq_off, eps_low, eps_high, beta, loss_type, max_completion_length=0, upstream=1.0):
    """fp64 replay of vlr_grpo_loss -> (stats dict, dlogp [R])"""
    lp = logp.double().clone().requires_grad_(True)
    dbl = lambda t: None if t is None else t.double()      # noqa: E731
    total, stats = loss(lp, dbl(old_logp), dbl(ref_logp), adv_seq.double(), seq_off, eps_low, eps_high, beta, loss_type, max_completion_length,
                        upstream)
    total.backward()
    return stats, lp.grad


def branch_counts(logp, old_logp, adv_seq, seq_off, eps_low, eps_high):
    """tokens per branch of the policy term, from the fp64 arithmetic -> dict under BRANCHES"""
    _, lens = _lens(seq_off)
    A = torch.repeat_interleave(adv_seq.double(), torch.tensor(lens))
    r = torch.exp(logp.double() - (logp if old_logp is None else old_logp).double())
    lo, hi = 1.0 - eps_low, 1.0 + eps_high
    inside = (r >= lo) & (r <= hi) & (A != 0)
    c_lo, c_hi = (r < lo) & (A < 0), (r > hi) & (A > 0)
    out = ((r < lo) & (A > 0)) | ((r > hi) & (A < 0))
    return dict(inside=int(inside.sum()), clipped_low=int(c_lo.sum()), clipped_high=int(c_hi.sum()), outside_unclipped=int(out.sum()),
                zero_advantage=int((A == 0).sum()))


def branch_inputs(lengths, adv_cycle, eps_low, eps_high, seed):
    """fp32 inputs of the loss that reach every branch: token i has ratio exactly 1 (logp == old; i % 3 == 0), a ratio inside the clip
    range and at least 0.02 from its bounds (i % 3 == 1), or one at least 0.05 outside, below and above in turn (i % 3 == 2) - so fp32
    and fp64 take the same branch everywhere.  Sequence s carries advantage adv_cycle[s % len(adv_cycle)].
    -> (logp, old_logp, ref_logp, adv_seq, seq_off)"""
    g = torch.Generator().manual_seed(seed)
    R = sum(lengths)
    seq_off = [0]
    for L in lengths:
        seq_off.append(seq_off[-1] + L)
    i = torch.arange(R)
    kind, up = i % 3, (i // 3) % 2 == 0
    x = torch.rand(R, generator=g)
    inside = torch.where(up, 1 + x * max(eps_high - 0.02, 0.0), 1 - x * max(eps_low - 0.02, 0.0))
    outside = torch.where(up, 1 + eps_high + 0.05 + 0.3 * x, 1 - eps_low - 0.05 - 0.3 * x)
    target = torch.where(kind == 0, torch.ones(R), torch.where(kind == 1, inside, outside))
    old = -torch.rand(R, generator=g) * 3
    logp = torch.where(kind == 0, old, old + torch.log(target))
    ref = logp + torch.randn(R, generator=g) * 0.3
    adv = torch.tensor([adv_cycle[s % len(adv_cycle)] for s in range(len(lengths))], dtype=torch.float32)
    return logp, old, ref, adv, seq_off


# ------------------------------------------------------------------------------------------------------------ the bounds
def _fold_depth(terms_per_lane):
    """additions an element passes through in a one-workgroup sum: its lane's running sum, 6 xor butterflies, 16 waves in order"""
    return terms_per_lane + 6 + 16


def advantage_bounds(scores, P, G, scale_rewards):
    """-> (fp64 replay (A, stats), per-element bound of A [P * G], bounds of the 3 stats).  The kernel takes the moments of d = s - s_0:
    d carries u |d|; the mean of d a lane-strided sum of ceil(G / 64) terms + 6 butterflies and the division; e = d - mean one more
    rounding; the variance the errors of e (Cauchy-Schwarz) and its own sum; sqrt and the division by std + 1e-4 three roundings."""
    s = scores.double().reshape(P, G)
    A, stats = advantages(scores.double(), P, G, scale_rewards)
    dep = math.ceil(G / 64) + 6
    d = s - s[:, :1]
    mean_abs_d, D = d.abs().mean(1, keepdim=True), d.abs().amax(1, keepdim=True)
    err_m = (2 * dep + 4) * U * mean_abs_d                     # of sum(d) / G
    err_e = err_m + 2 * U * D                                  # of one e = d - m
    e = s - s.mean(1, keepdim=True)
    sq = (e * e).sum(1, keepdim=True)
    var, std = sq / (G - 1), (sq / (G - 1)).sqrt()
    err_var = (2 * sq.sqrt() * math.sqrt(G) * err_e + G * err_e ** 2) / (G - 1) + (2 * dep + 6) * U * var
    err_std = torch.where(std > 0, err_var / std.clamp_min(1e-300), torch.zeros_like(std)) + 2 * U * std
    if scale_rewards:
        den = std + 1e-4
        b_A = err_e / den + A.reshape(P, G).abs() * (err_std / den + 4 * U)      # (1e-4 is rounded to fp32 once: within the 4 u)
    else:
        b_A = err_e + 0 * e
    gm = s.mean(1, keepdim=True)
    depP = _fold_depth(math.ceil(P / 16))
    b_mean = float((err_m + 2 * U * gm.abs()).mean() + (2 * depP + 4) * U * gm.abs().mean())
    b_std = float(err_std.mean() + (2 * depP + 4) * U * std.mean())
    return (A, stats), b_A.reshape(-1), torch.tensor([b_mean, b_std, 2 * U], dtype=torch.float64)


def check_advantages(got_A, got_stats, scores, P, G, scale_rewards):
    """a kernel's (advantages [P * G], stats [>= 3]) on fp32 `scores` against the fp64 replay -> (list of failures, worst error / bound)"""
    (A, stats), b_A, b_stats = advantage_bounds(scores, P, G, scale_rewards)
    fails, worst = [], 0.0
    if not bool(torch.isfinite(got_A.double()).all()):
        fails.append("advantages: not finite")
    err = (got_A.double() - A).abs()
    ratio = err / b_A.clamp_min(1e-300)
    flat = scores.double().reshape(P, G)
    equal = (flat == flat[:, :1]).all(1)                       # a group of equal scores: A = 0 EXACTLY, its std counted as 0 exactly
    if bool(equal.any()) and not bool((got_A.reshape(P, G)[equal] == 0).all()):
        fails.append("advantages: a group of equal scores is not exactly 0")
    live = ~equal.repeat_interleave(G)
    if bool(live.any()):
        worst = float(ratio[live].max())
        if not bool((err[live] <= b_A[live]).all()):
            i = int((ratio * live).argmax())
            fails.append(f"advantages[{i}]: got {float(got_A[i])!r} want {float(A[i])!r} err/bound {float(ratio[i]):.3g}")
    for i, name in enumerate(ADV_STAT_NAMES):
        e = abs(float(got_stats[i]) - float(stats[i]))
        worst = max(worst, e / max(float(b_stats[i]), 1e-300))
        if not e <= float(b_stats[i]):
            fails.append(f"stat {name}: got {float(got_stats[i])!r} want {float(stats[i])!r} err {e:.3g} bound {float(b_stats[i]):.3g}")
    if float(got_stats[2]) != float(torch.tensor(float(equal.sum()), dtype=torch.float32) / torch.tensor(float(P), dtype=torch.float32)):
        fails.append(f"stat frac_reward_zero_std: got {float(got_stats[2])!r}, {int(equal.sum())} of {P} groups have equal scores")
    return fails, worst


def loss_bounds(logp, old_logp, ref_logp, adv_seq, seq_off, eps_low, eps_high, beta, loss_type, max_completion_length=0, upstream=1.0):
    """-> (fp64 stats, fp64 dlogp, per-element bound of dlogp [R], dict of stat bounds).  Per token: x = logp - old carries u |x| into
    expf (2 ulp): the ratio to (|x| + 4) u; the products with A and the negation two more.  The KL term k = exp(d) - d - 1: exp(d) to
    (|d| + 4) u, two subtractions rounded at the magnitude of their operands (the cancellation near d = 0 is inside this ABSOLUTE bound),
    one fma with beta.  The weights 1 / (n len), 1 / R, 1 / (n max_completion_length) and upstream: four roundings.  Sums: no term passes
    through more additions than its lane's running sum (at most ceil(len / 64) terms per sequence of its wave: ceil(R / 64) + ceil(n /
    16) in all), 6 butterflies and 16 waves - twice for loss_type 0, whose sequence means are folded again."""
    lt = LOSS_TYPES.get(loss_type, loss_type)
    stats, dlogp = loss_and_grad(logp, old_logp, ref_logp, adv_seq, seq_off, eps_low, eps_high, beta, lt, max_completion_length, upstream)
    so, lens = _lens(seq_off)
    n, R = len(lens), logp.numel()
    lp = logp.double()
    old = lp if old_logp is None else old_logp.double()
    A = torch.repeat_interleave(adv_seq.double(), torch.tensor(lens))
    x = (lp - old).abs()
    r = torch.exp(lp - old)
    pol = torch.min(r * A, torch.clamp(r, 1.0 - eps_low, 1.0 + eps_high) * A).abs()
    err_tok = (x + 6) * U * pol
    mag_tok = pol.clone()
    err_g = (x + 8) * U * (A * r).abs()                        # of d l / d logp before the weight (0 where the reference's is 0: checked apart)
    k = torch.zeros_like(lp)
    err_k = torch.zeros_like(lp)
    if beta != 0:
        d = ref_logp.double() - lp
        ed = torch.exp(d)
        k = ed - d - 1.0
        err_k = (d.abs() + 4) * U * ed + U * d.abs() + 2 * U * (ed + d.abs() + 1)
        err_tok = err_tok + beta * err_k + 2 * U * (pol + beta * k.abs()) + U * beta * k.abs()
        mag_tok = mag_tok + beta * k.abs()
        err_g = err_g + beta * ((d.abs() + 6) * U * ed + 2 * U * (1 + ed)) + 2 * U * (A * r).abs()
    if lt == 0:
        w = torch.repeat_interleave(1.0 / (n * torch.tensor(lens, dtype=torch.float64)), torch.tensor(lens))
    elif lt == 1:
        w = torch.full((R,), 1.0 / R, dtype=torch.float64)
    else:
        w = torch.full((R,), 1.0 / (n * max_completion_length), dtype=torch.float64)
    depth = _fold_depth(math.ceil(R / 64) + math.ceil(n / 16)) * (2 if lt == 0 else 1)
    b_dlogp = abs(upstream) * w * err_g + 6 * U * dlogp.abs()
    tokmean = lambda e, m: float(e.mean() + (2 * depth + 4) * U * m.mean())      # noqa: E731
    b_stats = dict(loss=float((w * err_tok).sum() + (2 * depth + 8) * U * (w * mag_tok).sum()),
                   kl=tokmean(err_k, k.abs()), clip_low=4 * U, clip_high=4 * U, clip_region=10 * U,
                   ratio=tokmean((x + 4) * U * r, r), len_mean=2 * U * R / n)
    return stats, dlogp, b_dlogp, b_stats


def check_loss(got_dlogp, got_stats, logp, old_logp, ref_logp, adv_seq, seq_off, eps_low, eps_high, beta, loss_type, max_completion_length=0,
               upstream=1.0):
    """a kernel's (dlogp [R], stats [>= 7]) on fp32 inputs against the fp64 replay -> (list of failures, worst error / bound)"""
    stats, dlogp, b_dlogp, b_stats = loss_bounds(logp, old_logp, ref_logp, adv_seq, seq_off, eps_low, eps_high, beta, loss_type,
                                                 max_completion_length, upstream)
    fails = []
    got = got_dlogp.double()
    if not bool(torch.isfinite(got).all()):
        fails.append("dlogp: not finite")
    err = (got - dlogp).abs()
    ratio = err / b_dlogp.clamp_min(1e-300)
    worst = float(torch.where(dlogp == 0, torch.zeros_like(ratio), ratio).max())
    zero = dlogp == 0                                          # clipped side, A = 0: the gradient is EXACTLY 0 there (beta = 0)
    if beta == 0 and not bool(((got == 0) == zero).all()):
        i = int(((got == 0) != zero).nonzero()[0])
        fails.append(f"dlogp[{i}]: got {float(got[i])!r} want {float(dlogp[i])!r}: the exact zeros are not where autograd's are")
    bad = (err > b_dlogp) & ~(zero & (got == 0))
    if bool(bad.any()):
        i = int((ratio * bad).argmax())
        fails.append(f"dlogp[{i}]: got {float(got[i])!r} want {float(dlogp[i])!r} err/bound {float(ratio[i]):.3g}")
    for i, name in enumerate(STAT_NAMES):
        e = abs(float(got_stats[i]) - stats[name])
        worst = max(worst, e / max(b_stats[name], 1e-300))
        if not e <= b_stats[name]:
            fails.append(f"stat {name}: got {float(got_stats[i])!r} want {stats[name]!r} err {e:.3g} bound {b_stats[name]:.3g}")
    return fails, worst


# ------------------------------------------------------------------------------------------------------------ the policy through the oracles
def token_logps(W, cfg, pb, emulate=False, lora=None):
    """(token log-probs [R], seq_off [n + 1]) of the family's oracle forward on the response rows (tests/ppo_ref.py policy_heads, without
    the value head)"""
    from tests import ppo_ref as PR
    w, b = torch.zeros(cfg["hidden"]), torch.zeros(1)
    tok, _, seq_off = PR.policy_heads(W, cfg, pb, w, b, emulate, lora)
    return tok, seq_off


def _rows(pb, cfg, rows):
    """the batch rows `rows` (in that order) at the batch's padded width, with the images those rows name"""
    from tests import ppo_ref as PR
    return PR._rows(pb, cfg, rows)


def full_finetune_names(W):
    """what a full fine-tune trains on the HIP path (tests/ppo_ref.py train_steps): everything but the vision tower; of Qwen-VL's, the
    resampler without its fixed pos_embed stays trainable"""
    from oracle import llava_dpo_oracle as O
    ap = "transformer.visual.attn_pool."
    return [n for n in O.trainable_names(W) if not n.startswith("transformer.visual.") or (n.startswith(ap) and n != ap + "pos_embed")]


def step_grads(W, W_ref, cfg, pb, scores, P, G, hp, minibatches, names, upstream):
    """the gradient one backward batch of a full fine-tune leaves behind, in fp32 through the oracle: the reference pass and the
    advantages, then every minibatch (a list of rows, in generation order) at the SAME weights with old_logp = None (the first optimizer
    step of a step sees its own log-probs), its loss scaled by `upstream`, the gradients added.
    -> dict(ref, seq_off, advantages [P * G], adv_stats, stats [per minibatch], grads {name: grad})"""
    with torch.no_grad():
        ref_logp, seq_off = token_logps(W_ref, cfg, pb)
    A, a_stats = advantages(scores.double(), P, G, hp["scale_rewards"])
    A = A.float()
    leaves = {k: W[k].clone().requires_grad_(True) for k in names}
    Wl = dict(W)
    Wl.update(leaves)
    out = []
    for rows in minibatches:
        t0, t1 = seq_off[rows[0]], seq_off[rows[-1] + 1]
        so = [x - t0 for x in seq_off[rows[0]:rows[-1] + 2]]
        logp, _ = token_logps(Wl, cfg, _rows(pb, cfg, rows))
        total, st = loss(logp, None, ref_logp[t0:t1], A[rows], so, hp["epsilon"], hp["epsilon_high"], hp["beta"], hp["loss_type"],
                         hp.get("max_completion_length", 0), upstream)
        total.backward()
        out.append(st)
    return dict(ref=ref_logp, seq_off=seq_off, advantages=A, adv_stats=a_stats, stats=out, grads={k: v.grad for k, v in leaves.items()})


def train_steps(W, W_ref, cfg, pb, scores, P, G, hp, steps, num_iterations, mini_batch_size, lr, emulate=False, lora=None):
    """`steps` GRPO steps the way the HIP path stores things (tests/ppo_ref.py train_steps): fp32 master weights made from the bf16
    weights, every pass on their bf16 rounding, one Adam step (weight decay 0, no clipping) per minibatch, the rows in generation
    order, the old log-probs from a no-grad pass at the start of the step.  With `lora` only the adapters train and the reference is the
    adapter-free pass over the frozen base.  -> the per-minibatch stats dicts"""
    from oracle import llava_dpo_oracle as O
    names = full_finetune_names(W)
    master = {k: v.bfloat16().float() for k, v in W.items()}
    if lora is not None:
        names = list(lora["W"])
        master.update({k: v.bfloat16().float() for k, v in lora["W"].items()})
    with_lora = (lambda Wd: dict(lora, W={k: Wd[k] for k in lora["W"]})) if lora is not None else (lambda Wd: None)      # noqa: E731
    rnd = lambda: {k: v.bfloat16().float() for k, v in master.items()}      # noqa: E731
    state, out = {}, []
    N = P * G
    A = advantages(scores.double(), P, G, hp["scale_rewards"])[0].float()
    for _ in range(steps):
        Wp = rnd()
        with torch.no_grad():
            old_logp, seq_off = token_logps(Wp, cfg, pb, emulate, with_lora(Wp))
            ref_logp, _ = token_logps(W_ref if lora is None else Wp, cfg, pb, emulate)
        for _ in range(num_iterations):
            for m0 in range(0, N, mini_batch_size):
                rows = list(range(m0, m0 + mini_batch_size))
                t0, t1 = seq_off[m0], seq_off[m0 + mini_batch_size]
                so = [x - t0 for x in seq_off[m0:m0 + mini_batch_size + 1]]
                leaves = {k: Wp[k].clone().requires_grad_(True) for k in names}
                Wl = dict(Wp)
                Wl.update(leaves)
                logp, _ = token_logps(Wl, cfg, _rows(pb, cfg, rows), emulate, with_lora(Wl))
                total, st = loss(logp, old_logp[t0:t1], ref_logp[t0:t1], A[rows], so, hp["epsilon"], hp["epsilon_high"], hp["beta"],
                                 hp["loss_type"], hp.get("max_completion_length", 0))
                total.backward()
                grads = {k: v.grad for k, v in leaves.items() if v.grad is not None}
                with torch.no_grad():
                    O.adamw_step(master, grads, state, lr, 0.9, 0.999, 1e-8, 0.0)
                Wp = rnd()
                out.append(st)
    return out
