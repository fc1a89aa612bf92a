"""Checker side of the KTO tests: vlr_kto_loss of include/vlr.h ("KTO") restated in plain torch on the CPU.  The replay runs in fp64 on
the kernel's own fp32 inputs.  `loss` is ONE differentiable torch expression written as the header writes it (the KL baseline detached),
so the end-to-end tests get their gradients from torch autograd; `replay` is the closed form of the header, and the two agree
(tests/test_kto_checker_host.py).

check is the ONE comparison the GPU tests use: a kernel's outputs against the fp64 replay, within bounds derived from the fp32 unit
roundoff u = 2^-24, the number of terms a sum folds, the magnitude of the terms and expf's stated 2 ulp - never from a kernel's output.
tests/test_kto_checker_host.py plants faults and sees each of them flagged."""
import math

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126                                             # the smallest normal fp32: below it expf and the quotient may flush
STAT_NAMES = ("loss", "kl", "rewards_chosen_sum", "rewards_rejected_sum", "logps_chosen_sum", "logps_rejected_sum", "count_chosen",
              "count_rejected")
BRANCHES = ("desirable_flat", "desirable_mid", "desirable_saturated", "undesirable_flat", "undesirable_mid", "undesirable_saturated")
SAT_HI, SAT_LO = 89.0, -104.0                                  # expf overflows fp32 above 88.73 and is 0 below -103.98


def _d(t):
    return torch.as_tensor(t).double()


def _f32(x):
    """a scalar as the C ABI hands it to the kernel: rounded to fp32 once"""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _w(lab, w_d, w_u):
    return torch.where(lab, torch.tensor(w_d, dtype=torch.float64), torch.tensor(w_u, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------------------ the arithmetic
def loss(pi, ref, label, pi_kl, ref_kl, beta, w_d, w_u, upstream=1.0):
    """vlr_kto_loss as ONE differentiable torch expression in the dtype of `pi` -> (loss * upstream with its graph, kl, losses [n],
    rewards [n]).  The KL baseline is detached: no gradient flows into it."""
    kl = (pi_kl - ref_kl).mean().clamp(min=0).detach()
    r = pi - ref
    lab = torch.as_tensor(label).bool()
    losses = torch.where(lab, w_d * (1 - torch.sigmoid(beta * (r - kl))), w_u * (1 - torch.sigmoid(beta * (kl - r))))
    return losses.mean() * upstream, kl, losses, beta * r


def replay(pi, ref, label, pi_kl, ref_kl, beta, w_d, w_u, upstream=1.0):
    """fp64 closed form of the header -> dict(losses, rewards, dpi, z, q = 1 - sigmoid(z), s = sigmoid(z) [n], stats [8] under STAT_NAMES)"""
    pi, ref, pi_kl, ref_kl = _d(pi), _d(ref), _d(pi_kl), _d(ref_kl)
    beta, w_d, w_u, upstream = _f32(beta), _f32(w_d), _f32(w_u), _f32(upstream)
    lab = torch.as_tensor(label).bool()
    n = pi.numel()
    kl = max(0.0, float((pi_kl - ref_kl).sum()) / pi_kl.numel())
    r = pi - ref
    z = torch.where(lab, beta * (r - kl), beta * (kl - r))
    ez = torch.exp(-z.abs())
    q = torch.where(z > 0, ez / (1 + ez), 1 / (1 + ez))       # 1 - sigmoid(z) and sigmoid(z), each without a cancellation
    sg = torch.where(z > 0, 1 / (1 + ez), ez / (1 + ez))
    w = _w(lab, w_d, w_u)
    losses = w * q
    rewards = beta * r
    sign = _w(lab, -1.0, 1.0)
    dpi = sign * (w * beta / n) * q * sg * upstream
    f = lab.double()
    stats = torch.stack([losses.sum() / n, torch.tensor(kl).double(), (rewards * f).sum(), (rewards * (1 - f)).sum(), (pi * f).sum(),
                         (pi * (1 - f)).sum(), f.sum(), (1 - f).sum()])
    return dict(losses=losses, rewards=rewards, dpi=dpi, z=z, q=q, s=sg, stats=stats, kl=kl)


def branch_counts(pi, ref, label, pi_kl, ref_kl, beta):
    """rows per branch from the fp64 arithmetic: the label, and |z| below 1 / up to the saturation of expf / beyond it"""
    rp = replay(pi, ref, label, pi_kl, ref_kl, beta, 1.0, 1.0)
    lab = torch.as_tensor(label).bool()
    z = rp["z"]
    sat = (z > SAT_HI) | (z < SAT_LO)
    flat = z.abs() < 1
    out = {}
    for name, sel in (("desirable", lab), ("undesirable", ~lab)):
        out[name + "_flat"] = int((sel & flat).sum())
        out[name + "_mid"] = int((sel & ~flat & ~sat).sum())
        out[name + "_saturated"] = int((sel & sat).sum())
    return out


def make_inputs(n, m, labels, beta, kl_mean, seed):
    """fp32 inputs that reach every branch.  labels: "ones", "zeros" or "mixed".  The KL rows have log-ratios around kl_mean (negative:
    the clamp is hit).  Row i aims at beta (r - kl) = Z[i % 8] for Z = 0.25, -1, 1, -30, 30, -200, 200, -0.5 - flat, around 1, at 30 and
    saturated, on both sides.  -> (pi, ref, label [n] uint8, pi_kl, ref_kl)"""
    g = torch.Generator().manual_seed(seed)
    ref_kl = -20 - 200 * torch.rand(m, generator=g)
    pi_kl = ref_kl + kl_mean + 0.5 * (torch.rand(m, generator=g) - 0.5)
    kl = max(0.0, float((pi_kl.double() - ref_kl.double()).mean()))
    i = torch.arange(n)
    Z = torch.tensor([0.25, -1.0, 1.0, -30.0, 30.0, -200.0, 200.0, -0.5])[i % 8] * (1 + 0.1 * torch.rand(n, generator=g))
    if labels == "ones":
        label = torch.ones(n, dtype=torch.uint8)
    elif labels == "zeros":
        label = torch.zeros(n, dtype=torch.uint8)
    else:
        label = ((i // 8 + i) % 2).to(torch.uint8)            # alternating, shifted by one every 8 rows: both labels on every z target
    ref = -20 - 200 * torch.rand(n, generator=g)
    pi = ref + (kl + Z / beta)
    return pi, ref, label, pi_kl, ref_kl


# ------------------------------------------------------------------------------------------------------------ the bounds
def _fold_depth(rows):
    """additions an element passes through in the one-workgroup sum: its lane's running sum (1024 lanes stride the rows), 6 xor
    butterflies, 16 waves in order"""
    return math.ceil(rows / 1024) + 6 + 16


def bounds(pi, ref, label, pi_kl, ref_kl, beta, w_d, w_u, upstream=1.0):
    """-> (replay dict, dict of per-element bounds losses / rewards / dpi [n], bounds of the 8 stats [8]).
    kl: the mean over m is bounded by m u max|pi_kl - ref_kl| (each difference one rounding, no element passes through more than m
    additions, the division one more - for the m the tests use, 1 and >= 64, that is within m u max|d|); the clamp is 1-Lipschitz.
    Per row: r = pi - ref carries u |r|; a = r - kl carries that, kl's error and u |a|; z = beta a one more rounding.  expf (2 ulp = 4 u)
    turns the absolute error of z into a relative one of e; q = 1 / (1 + e) has relative error s rel(e) + 2 u with s = e / (1 + e) (one
    addition, one division), the second-order terms below one more u (rel(e) < 2^-12 is asserted); where e overflows or the quotient
    underflows q may flush to 0: an absolute 2^-126.  loss = w q: one rounding.  1 - q: q's absolute error and one rounding; q (1 - q)
    one more; the weight ((w beta) / n) upstream three roundings and the product a fourth.  reward = beta r: u |r| scaled and one
    rounding.  Sums: a term passes through at most ceil(rows / 1024) + 22 additions; the loss mean one division more.  The counts are
    sums of ones below 2^24: exact."""
    rp = replay(pi, ref, label, pi_kl, ref_kl, beta, w_d, w_u, upstream)
    pi_, ref_ = _d(pi), _d(ref)
    lab = torch.as_tensor(label).bool()
    n, m = pi_.numel(), _d(pi_kl).numel()
    ab = abs(_f32(beta))
    err_kl = m * U * float((_d(pi_kl) - _d(ref_kl)).abs().max())
    r = pi_ - ref_
    a = (r - rp["kl"]).abs()
    err_z = ab * (U * r.abs() + err_kl + U * a) + U * rp["z"].abs()
    rel_e = torch.expm1(err_z) + 4 * U
    assert float(rel_e.max()) < 2.0 ** -12, "the first-order bound of q needs rel(e) < 2^-12"
    q, s = rp["q"], rp["s"]
    b_q = (s * rel_e + 3 * U) * q + TINY
    w = _w(lab, _f32(w_d), _f32(w_u)).abs()
    b_loss = w * b_q + U * w * q
    g0 = q * s
    b_g0 = b_q * s + q * (b_q + U * s) + U * g0
    c = w * ab / n * abs(_f32(upstream))
    b_dpi = c * b_g0 + 4 * U * c * g0
    b_rw = ab * U * r.abs() + U * ab * r.abs()
    D = _fold_depth(n)
    f = lab.double()
    b_stats = torch.stack([
        b_loss.sum() / n + (D + 2) * U * (w * q).sum() / n,
        torch.tensor(err_kl).double(),
        (b_rw * f).sum() + D * U * (rp["rewards"].abs() * f).sum(),
        (b_rw * (1 - f)).sum() + D * U * (rp["rewards"].abs() * (1 - f)).sum(),
        D * U * (pi_.abs() * f).sum(),
        D * U * (pi_.abs() * (1 - f)).sum(),
        torch.tensor(0.0).double(), torch.tensor(0.0).double()])
    return rp, dict(losses=b_loss, rewards=b_rw, dpi=b_dpi), b_stats


def check(got_losses, got_rewards, got_dpi, got_stats, pi, ref, label, pi_kl, ref_kl, beta, w_d, w_u, upstream=1.0):
    """a kernel's (losses, rewards, dpi [n], stats [8]) on fp32 inputs against the fp64 replay -> (list of failures, worst error /
    bound).  Beyond the bounds: everything is finite; a KL mean that is negative beyond its bound gives kl == 0 EXACTLY; a row whose z is
    past the saturation of expf has loss exactly 0 (z > 89) or exactly fp32(w) (z < -104) and gradient exactly 0; the counts are exact."""
    rp, b, b_stats = bounds(pi, ref, label, pi_kl, ref_kl, beta, w_d, w_u, upstream)
    fails, worst = [], 0.0
    got = dict(losses=_d(got_losses), rewards=_d(got_rewards), dpi=_d(got_dpi))
    gs = _d(got_stats)
    for name in ("losses", "rewards", "dpi"):
        if not bool(torch.isfinite(got[name]).all()):
            fails.append(f"{name}: not finite")
            continue
        err = (got[name] - rp[name]).abs()
        ratio = err / b[name].clamp_min(1e-300)
        live = b[name] > TINY * 4                              # rows whose bound is the flush floor alone say nothing as a ratio
        if bool(live.any()):
            worst = max(worst, float(ratio[live].max()))
        bad = err > b[name]
        if bool(bad.any()):
            i = int((ratio * bad).argmax())
            fails.append(f"{name}[{i}]: got {float(got[name][i])!r} want {float(rp[name][i])!r} err/bound {float(ratio[i]):.3g}")
    if not bool(torch.isfinite(gs[:8]).all()):
        fails.append("stats: not finite")
    for i, name in enumerate(STAT_NAMES):
        e = abs(float(gs[i]) - float(rp["stats"][i]))
        if float(b_stats[i]) > 0:
            worst = max(worst, e / float(b_stats[i]))
        if not e <= float(b_stats[i]):
            fails.append(f"stat {name}: got {float(gs[i])!r} want {float(rp['stats'][i])!r} err {e:.3g} bound {float(b_stats[i]):.3g}")
    mean64 = float((_d(pi_kl) - _d(ref_kl)).sum()) / _d(pi_kl).numel()
    if mean64 < -float(b_stats[1]) and float(gs[1]) != 0.0:
        fails.append(f"stat kl: got {float(gs[1])!r} for a KL mean of {mean64!r}: not clamped at 0")
    lab = torch.as_tensor(label).bool()
    w32 = _w(lab, _f32(w_d), _f32(w_u))
    hi, lo = rp["z"] > SAT_HI, rp["z"] < SAT_LO
    if bool(hi.any()) and not (bool((got["losses"][hi] == 0).all()) and bool((got["dpi"][hi] == 0).all())):
        fails.append("saturated rows (z > 89): loss and gradient are not exactly 0")
    if bool(lo.any()) and not (bool((got["losses"][lo] == w32[lo]).all()) and bool((got["dpi"][lo] == 0).all())):
        fails.append("saturated rows (z < -104): loss is not exactly w or the gradient not exactly 0")
    return fails, worst


# ------------------------------------------------------------------------------------------------------------ the policy through the oracles
def seq_logps(W, cfg, pb, emulate=False, lora=None):
    """summed completion log-probs [rows] of the family's oracle forward (tests/grpo_ref.py token_logps, summed per sequence)"""
    from tests import grpo_ref as GR
    tok, seq_off = GR.token_logps(W, cfg, pb, emulate, lora)
    return torch.stack([tok[seq_off[i]:seq_off[i + 1]].sum() for i in range(len(seq_off) - 1)])


def batch_loss(Wp, W_ref, cfg, main, klb, label, beta, w_d, w_u, upstream=1.0, emulate=False, lora=None, lora_nograd=None):
    """one KTO batch through the family's oracle: main / klb are the oracle batches of the main rows and of their KL rows.  The policy
    is Wp (with `lora` where given); the reference is W_ref, or under LoRA the adapter-free pass over Wp's base (W_ref None); the KL rows
    run without a graph (with `lora_nograd`, the adapters detached).
    -> (loss * upstream with its graph, dict(loss, kl, pi, pi_kl, ref, ref_kl))"""
    pi = seq_logps(Wp, cfg, main, emulate, lora)
    with torch.no_grad():
        pi_kl = seq_logps({k: v.detach() for k, v in Wp.items()}, cfg, klb, emulate, lora_nograd if lora is not None else None)
        Wr = W_ref if W_ref is not None else {k: v.detach() for k, v in Wp.items()}
        ref, ref_kl = seq_logps(Wr, cfg, main, emulate), seq_logps(Wr, cfg, klb, emulate)
    total, kl, _, _ = loss(pi, ref, label, pi_kl, ref_kl, beta, w_d, w_u, upstream)
    return total, dict(loss=float(total.detach()) / upstream, kl=float(kl), pi=pi.detach(), pi_kl=pi_kl, ref=ref, ref_kl=ref_kl)


def train_steps(W, W_ref, cfg, batches, beta, w_d, w_u, steps, lr, emulate=False, lora=None):
    """`steps` optimizer steps, each over ALL of `batches` (a list of (main, klb, label)) accumulated with weight 1 / len(batches), the way
    the HIP path stores things (tests/grpo_ref.py train_steps): fp32 master weights made from the bf16 weights, every pass on their bf16
    rounding, one Adam step (betas 0.9 / 0.999, eps 1e-8, weight decay 0, no clipping) per step.  With `lora` only the adapters train and
    the reference is the adapter-free pass over the frozen base.
    -> (the per-minibatch losses, in order; the norm of every step's accumulated gradient)"""
    from oracle import llava_dpo_oracle as O
    from tests import grpo_ref as GR
    names = GR.full_finetune_names(W)
    master = {k: v.bfloat16().float() for k, v in W.items()}
    if lora is not None:
        names = list(lora["W"])
        master.update({k: v.bfloat16().float() for k, v in lora["W"].items()})
    with_lora = (lambda Wd: dict(lora, W={k: Wd[k] for k in lora["W"]})) if lora is not None else (lambda Wd: None)      # noqa: E731
    state, out, norms = {}, [], []
    for _ in range(steps):
        Wp = {k: v.bfloat16().float() for k, v in master.items()}
        leaves = {k: Wp[k].clone().requires_grad_(True) for k in names}
        Wl = dict(Wp)
        Wl.update(leaves)
        for main, klb, label in batches:
            total, st = batch_loss(Wl, W_ref if lora is None else None, cfg, main, klb, label, beta, w_d, w_u, 1.0 / len(batches), emulate,
                                   with_lora(Wl), with_lora(Wp))
            total.backward()
            out.append(st["loss"])
        grads = {k: v.grad for k, v in leaves.items() if v.grad is not None}
        norms.append(math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads.values())))
        with torch.no_grad():
            O.adamw_step(master, grads, state, lr, 0.9, 0.999, 1e-8, 0.0)
    return out, norms
