"""Checker side of the entropy tests: the row entropy of the fused lm-head (include/vlr.h, vlr_lmhead_logps_entropy_fwd / _bwd) and
vlr_grpo_loss_ent restated on the host.  The reference is fp64 on the logits hg.double() @ w.double().T; every bound is a formula of
the number formats and of the reference itself, never of a kernel's output:

  logits      the kernels accumulate H exact bf16 x bf16 products in fp32, in any order: |dz[r][v]| <= (H + 4) u (|hg| |w|^T)[r][v],
              u = 2^-24.
  entropy     dH / dz_v = -p_v (log p_v + H): the logit errors reach the entropy through sum_v p_v |log p_v + H| |dz_v| (the row's
              Lipschitz bound, element by element), second order (max dz)^2 (2 + log V).  The arithmetic: a term e^(z - M) passes through
              two __expf (rel. (2 |x| + 8) u each: the product with log2 e carries |x| u, the hardware exponential and the rounding of
              its argument the rest; the two arguments add up to z - M) and at most DEPTH(V) additions, so S = sum e^(z - M) is relative
              eps_S = sum_v p_v d_v, d_v = (2 |z_v - M| + 16 + DEPTH) u; T = sum e^(z - M) (z - M) has every term <= 0 (nothing cancels) and
              is off by sum e^(z - M) |z - M| (d_v + 4 u); H = log S - T / S adds logf's 2 ulp, the division and the subtraction.
  lse         sum_v p_v |dz_v| + eps_S + 3 u |lse|.
  d logits    the backward is handed the kernel's own lse and H (within the two bounds above of the reference's) and recomputes z:
              log p = z - lse is off by e_lp = |dz_v| + b_lse, p relatively by e_lp + (2 |log p| + 8) u; both terms are propagated
              through  dlogp ([v == tgt] - p) - dent (p (log p + H))  with four roundings each, then ONE bf16
              rounding (8 significant bits: 2^-8 relative; 2^-126 absolute where fp32 denormals are flushed).

replay_forward / replay_backward are a numpy fp32 restatement of the partial / fold scheme with switches that plant faults;
tests/test_entropy_checker_host.py shows that the checks accept the correct replay and flag each fault."""
import math

import numpy as np
import torch

from tests import grpo_ref as GR

U = 2.0 ** -24
BF16 = 2.0 ** -8              # bf16's unit roundoff: 8 significant bits, round to nearest -> half an ulp is 2^-8 of the value at most
# (R, V, H, fused on the MI355X's 256 compute units?)
SHAPES = [(2100, 8200, 512, True), (2304, 32064, 256, True), (300, 512, 128, False), (3, 1032, 64, False), (1, 8, 8, False)]
N_RESERVED = 7               # features 0..6 of hg / w carry the planted rows when H >= 16


def depth(V):
    """additions a term of a row's sums passes through, at most: the row kernel's lane (4 per 1024-column stride), 6 butterflies and 4
    waves - the fused route's 16 accumulator elements, 2 butterflies, ceil(V / 4096) parts per lane of the fold and 6 butterflies are fewer"""
    return 4 * math.ceil(V / 1024) + 16


def dominant_columns(V):
    """where a row's dominant logit is planted: column 0, both sides of the first 256-column tile edge, inside the last (partial when
    V % 256 != 0) column tile, the last column"""
    last0 = ((V - 1) // 256) * 256
    cols = [0, 255, 256, last0 + (V - last0) // 2, V - 1]
    out = []
    for c in cols:
        if 0 <= c < V and c not in out:
            out.append(c)
    return out


def make_case(R, V, H, seed, device="cpu"):
    """bf16 operands with the planted rows in front -> dict(hg [R][H], w [V][H], tgt [R] int32, kinds [R] list of names).
    Rows (as many as fit beside at least one random row, none when H < 16): 'zero' - hg = 0, every logit 0, H = log V; 'dom@c' - the
    target column c beats every other logit by 128 (H = 0 within the bound, never NaN); 'tie' - two equal maxima 8 above the rest in
    different 256-column tiles (different 1024-column strides of the row kernel when V > 1024); the rest random."""
    g = torch.Generator().manual_seed(seed)
    hg = torch.randn(R, H, generator=g)
    w = torch.randn(V, H, generator=g) * 0.2
    tgt = torch.randint(0, V, (R,), generator=g, dtype=torch.int32)
    kinds = ["random"] * R
    if H >= 16:
        doms = dominant_columns(V)[:N_RESERVED - 1]
        hg[:, :N_RESERVED] = 0
        w[:, :N_RESERVED] = 0
        plan = ["tie"] + [f"dom@{c}" for c in reversed(doms)] + ["zero"]          # a short R keeps the far columns and the tie
        plan = plan[:max(R - 1, 0)] if R <= len(plan) else plan
        for j, c in enumerate(doms):
            w[c, j] = 16.0
        c2 = V - 2 if V > 2 else V - 1
        w[1, N_RESERVED - 1] = 4.0
        w[c2, N_RESERVED - 1] = 4.0
        for r, kind in enumerate(plan):
            hg[r] = 0
            if kind == "tie":
                hg[r, N_RESERVED - 1] = 2.0
                tgt[r] = c2
            elif kind.startswith("dom@"):
                c = int(kind[4:])
                hg[r, doms.index(c)] = 8.0
                tgt[r] = c
            kinds[r] = kind
    if R > len([k for k in kinds if k != "random"]) + 4:
        base = R - 4
        tgt[base:base + 4] = torch.tensor([0, V - 1, min(255, V - 1), min(256, V - 1)], dtype=torch.int32)      # random rows whose TARGET sits on the edges
    return dict(hg=hg.bfloat16().to(device), w=w.bfloat16().to(device), tgt=tgt.to(device), kinds=kinds)


# ------------------------------------------------------------------------------------------------------------ the fp64 reference
def _chunks(R, V):
    step = max(1, min(R, (1 << 23) // V))
    return [(a, min(a + step, R)) for a in range(0, R, step)]


def _logits(hg, w, a, b):
    """fp64 logits of rows a..b and their error bound (H + 4) u |hg| |w|^T"""
    x = hg[a:b].double()
    wd = w.double()
    z = x @ wd.t()
    ez = (hg.shape[1] + 4) * U * (x.abs() @ wd.abs().t())
    return z, ez


def _row_terms(z, ez, V):
    M = z.max(1, keepdim=True).values
    lse = torch.logsumexp(z, 1, keepdim=True)
    lp = z - lse
    p = torch.exp(lp)
    Hh = -(p * lp).sum(1, keepdim=True)
    S = torch.exp(lse - M)
    d = (2 * (z - M).abs() + 16 + depth(V)) * U
    eps_S = (p * d).sum(1, keepdim=True)
    T_abs = (p * (z - M).abs()).sum(1, keepdim=True)                                    # |T| / S
    lip = (p * (lp + Hh).abs() * ez).sum(1, keepdim=True)
    emax = ez.max(1, keepdim=True).values
    b_H = lip * (1 + 4 * emax) + emax ** 2 * (2 + math.log(V)) + eps_S + 3 * U * torch.log(S).abs() \
        + (p * (z - M).abs() * (d + 4 * U)).sum(1, keepdim=True) + T_abs * (eps_S + 2 * U) + 2 * U * Hh.abs()
    b_lse = (p * ez).sum(1, keepdim=True) * (1 + emax) + eps_S + 3 * U * lse.abs()
    return lse, lp, p, Hh, b_H, b_lse


def forward_reference(hg, w, tgt):
    """-> dict of fp64 [R] tensors on hg's device: lse, tok (log-prob of the target), H, b_H, b_lse, b_tok, and the row's largest logit
    error ez"""
    R, V = hg.shape[0], w.shape[0]
    out = {k: [] for k in ("lse", "tok", "H", "b_H", "b_lse", "b_tok", "ez")}
    for a, b in _chunks(R, V):
        z, ez = _logits(hg, w, a, b)
        lse, lp, p, Hh, b_H, b_lse = _row_terms(z, ez, V)
        t = tgt[a:b].long()[:, None]
        out["lse"].append(lse[:, 0])
        out["tok"].append(lp.gather(1, t)[:, 0])
        out["H"].append(Hh[:, 0])
        out["b_H"].append(b_H[:, 0])
        out["b_lse"].append(b_lse[:, 0])
        out["b_tok"].append((b_lse + ez.gather(1, t) + 2 * U * (z.gather(1, t).abs() + lse.abs()))[:, 0])
        out["ez"].append(ez.max(1).values)
    return {k: torch.cat(v) for k, v in out.items()}


def check_entropy(got_H, ref, V, what="entropy"):
    """a kernel's entropy [R] against forward_reference -> (failures, worst error / bound).  Also: finite, and inside
    [-bound, log V + bound]"""
    got = got_H.double().to(ref["H"].device)
    fails = []
    if not bool(torch.isfinite(got).all()):
        fails.append(f"{what}: not finite at row {int((~torch.isfinite(got)).nonzero()[0])}")
        got = torch.nan_to_num(got, nan=1e30, posinf=1e30, neginf=-1e30)
    err = (got - ref["H"]).abs()
    ratio = err / ref["b_H"]
    if not bool((err <= ref["b_H"]).all()):
        i = int(ratio.argmax())
        fails.append(f"{what}[{i}]: got {float(got[i])!r} want {float(ref['H'][i])!r} err {float(err[i]):.3g} bound {float(ref['b_H'][i]):.3g}")
    out = (got < -ref["b_H"]) | (got > math.log(V) + ref["b_H"])
    if bool(out.any()):
        i = int(out.nonzero()[0])
        fails.append(f"{what}[{i}]: {float(got[i])!r} outside [0, log V] by more than the bound")
    return fails, float(ratio.max())


def backward_reference(z, ez, b_lse, b_H, lse, Hh, tgt, dlogp, dent):
    """fp64 d logits of one row block and its bound.  z, ez [r][V]; lse, Hh the fp64 reference's [r][1]; b_lse, b_H [r][1] how far the lse
    and entropy the kernel is handed may sit from them; dlogp, dent [r][1] fp64"""
    lp = z - lse
    p = torch.exp(lp)
    ind = torch.zeros_like(z)
    ind.scatter_(1, tgt.long()[:, None], 1.0)
    t0 = dlogp * (ind - p)
    t1 = dent * (p * (lp + Hh))
    d = t0 - t1
    e_lp = ez + b_lse + 2 * U * (z.abs() + lse.abs())
    rel_p = e_lp * (1 + e_lp) + (2 * lp.abs() + 8) * U
    b0 = dlogp.abs() * (p * rel_p + 2 * U * (ind - p).abs()) + 2 * U * t0.abs()
    b1 = dent.abs() * p * (rel_p * (lp + Hh).abs() + e_lp + b_H + 2 * U * (lp.abs() + Hh.abs())) + 4 * U * t1.abs()
    b = (b0 + b1 + U * d.abs()) * (1 + BF16) + BF16 * d.abs() + 2.0 ** -126
    return d, b


def check_dlogits(got_dl, hg, w, tgt, ref, dlogp, dent, what="dlogits"):
    """a kernel's d logits (bf16 [R][>= V], the first V columns) against the fp64 formula on the reference's lse and entropy, the kernel
    having been handed lse and entropy within ref's bounds -> (failures, worst error / bound)"""
    R, V = hg.shape[0], w.shape[0]
    dev = hg.device
    fails, worst = [], 0.0
    col = lambda t, a, b: t[a:b].double().to(dev)[:, None]      # noqa: E731
    for a, b in _chunks(R, V):
        z, ez = _logits(hg, w, a, b)
        d, bd = backward_reference(z, ez, col(ref["b_lse"], a, b), col(ref["b_H"], a, b), col(ref["lse"], a, b), col(ref["H"], a, b),
                                   tgt[a:b], col(dlogp, a, b), col(dent, a, b))
        got = got_dl[a:b, :V].double().to(dev)
        if not bool(torch.isfinite(got).all()):
            fails.append(f"{what}: not finite in rows {a}..{b}")
            got = torch.nan_to_num(got, nan=1e30, posinf=1e30, neginf=-1e30)
        err = (got - d).abs()
        ratio = err / bd
        worst = max(worst, float(ratio.max()))
        if not bool((err <= bd).all()):
            i = int(ratio.argmax())
            r, c = a + i // V, i % V
            fails.append(f"{what}[{r}][{c}]: got {float(got[i // V, c])!r} want {float(d[i // V, c])!r} err/bound {float(ratio.reshape(-1)[i]):.3g}")
    return fails, worst


# ------------------------------------------------------------------------------------------------------------ the fp32 replay, with faults
FWD_FAULTS = ("drop_shift", "own_max", "skip_last_tile", "unmasked_last_tile")
BWD_FAULTS = ("no_H", "flip_dent")


def replay_forward(hg, w, tgt, fault=None):
    """numpy fp32 restatement of the fuse = 8 epilogue and its fold: (m, s, t) per row and 64-column part (the wave's columns wc * 32 ..
    + 32 of both 128-column halves of a 256-column tile), folded over the parts in order -> (tok_logp, lse, H) fp32 [R].
    fault: 'drop_shift' - the (m_i - M) s_i term missing from T; 'own_max' - a part's own maximum in place of the global one (S = sum s_i,
    T = sum t_i); 'skip_last_tile' - the last partial column tile never folded; 'unmasked_last_tile' - its columns >= V (zero logits)
    counted."""
    f32 = np.float32
    z = (hg.float().cpu() @ w.float().cpu().t()).numpy().astype(f32)
    R, V = z.shape
    tiles = (V + 255) // 256
    partial = V % 256 != 0
    ms, ss, ts = [], [], []
    for tile in range(tiles):
        last = tile == tiles - 1 and partial
        if last and fault == "skip_last_tile":
            continue
        for wc in range(4):
            cols = np.concatenate([np.arange(32) + tile * 256 + b * 128 + wc * 32 for b in range(2)])
            if last and fault == "unmasked_last_tile":
                zz = np.zeros((R, 64), f32)
                ok = cols < V
                zz[:, ok] = z[:, cols[ok]]
            else:
                cols = cols[cols < V]
                if cols.size == 0:
                    ms.append(np.full(R, -np.inf, f32)), ss.append(np.zeros(R, f32)), ts.append(np.zeros(R, f32))
                    continue
                zz = z[:, cols]
            m = zz.max(1)
            d = (zz - m[:, None]).astype(f32)
            e = np.exp(d).astype(f32)
            ms.append(m), ss.append(e.sum(1, dtype=f32)), ts.append((e * d).sum(1, dtype=f32))
    m, s, t = np.stack(ms, 1), np.stack(ss, 1), np.stack(ts, 1)
    M = m.max(1, keepdims=True)
    with np.errstate(invalid="ignore"):
        dm = np.where(np.isfinite(m), m - M, f32(0)).astype(f32)
    sc = np.where(np.isfinite(m), np.exp(dm), f32(0)).astype(f32)
    if fault == "own_max":
        sc = np.isfinite(m).astype(f32)
    S = (s * sc).sum(1, dtype=f32)
    T = (sc * (t if fault == "drop_shift" or fault == "own_max" else t + dm * s)).sum(1, dtype=f32)
    ls = np.log(S).astype(f32)
    lse = (M[:, 0] + ls).astype(f32)
    tok = z[np.arange(R), tgt.cpu().numpy().astype(np.int64)] - lse
    return torch.from_numpy(tok.astype(f32)), torch.from_numpy(lse), torch.from_numpy((ls - T / S).astype(f32))


def replay_backward(hg, w, tgt, lse, Hh, dlogp, dent, fault=None):
    """numpy fp32 restatement of the fuse = 9 epilogue -> bf16 [R][V].  fault: 'no_H' - the H_r term missing; 'flip_dent' - the entropy
    term added instead of subtracted"""
    z = hg.float().cpu() @ w.float().cpu().t()
    zl = z - lse.float().cpu()[:, None]
    p = torch.exp(zl)
    ind = torch.zeros_like(z)
    ind.scatter_(1, tgt.cpu().long()[:, None], 1.0)
    t0 = dlogp.float().cpu()[:, None] * (ind - p)
    h = torch.zeros_like(Hh) if fault == "no_H" else Hh
    t1 = dent.float().cpu()[:, None] * (p * (zl + h.float().cpu()[:, None]))
    return (t0 + t1 if fault == "flip_dent" else t0 - t1).bfloat16()


# ------------------------------------------------------------------------------------------------------------ vlr_grpo_loss_ent
ENT_STAT_NAMES = GR.STAT_NAMES + ("zero", "entropy", "kept_frac")


def grpo_ent_loss(logp, old_logp, ref_logp, adv_seq, seq_off, eps_low, eps_high, beta, loss_type, max_completion_length, upstream, entropy,
                  keep, entropy_coef):
    """vlr_grpo_loss_ent as ONE differentiable torch expression in the dtype of `logp` -> (loss * upstream with its graph, stats dict).
    entropy [R] (may carry a graph) or None, keep [R] bool / 0-1 or None.  The KL, clip and ratio statistics are over all R tokens."""
    lt = GR.LOSS_TYPES.get(loss_type, loss_type)
    so, lens = GR._lens(seq_off)
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
    k = torch.ones_like(tok) if keep is None else keep.to(logp.dtype)
    Hh = torch.zeros_like(tok) if entropy is None else entropy.to(logp.dtype)
    tok = k * tok - entropy_coef * Hh
    if lt == 0:
        total = sum(tok[so[s]:so[s + 1]].sum() / lens[s] for s in range(n)) / n
    elif lt == 1:
        total = tok.sum() / R
    else:
        total = tok.sum() / (n * max_completion_length)
    low = ((r < 1.0 - eps_low) & (A < 0)).to(logp.dtype).mean()
    high = ((r > 1.0 + eps_high) & (A > 0)).to(logp.dtype).mean()
    stats = dict(loss=total, kl=kl.mean(), clip_low=low, clip_high=high, clip_region=low + high, ratio=r.mean(), len_mean=torch.tensor(R / n),
                 zero=torch.tensor(0.0), entropy=Hh.mean(), kept_frac=k.mean())
    return total * upstream, {kk: float(v.detach()) for kk, v in stats.items()}


def check_grpo_ent(got_dlogp, got_dent, got_stats, logp, old_logp, ref_logp, adv_seq, seq_off, eps_low, eps_high, beta, loss_type,
                   max_completion_length, upstream, entropy, keep, entropy_coef):
    """a kernel's (dlogp [R], dent [R], stats [10]) against the fp64 replay -> (failures, worst error / bound).  The bounds of dlogp and of
    stats[1..6] are grpo_ref.loss_bounds' (the statements are vlr_grpo_loss's); the loss adds the bonus - sum_t w_t coef H_t: a product
    and the same fold depth; a masked token's dlogp is EXACTLY 0; dent = -coef upstream w_t, six roundings."""
    dbl = lambda t: None if t is None else t.double()      # noqa: E731
    lp = logp.double().clone().requires_grad_(True)
    Hd = None if entropy is None else entropy.double().clone().requires_grad_(True)
    total, stats = grpo_ent_loss(lp, dbl(old_logp), dbl(ref_logp), adv_seq.double(), seq_off, eps_low, eps_high, beta, loss_type,
                                 max_completion_length, upstream, Hd, keep, entropy_coef)
    total.backward()
    dlogp = lp.grad
    dent = torch.zeros_like(dlogp) if Hd is None or Hd.grad is None else Hd.grad
    _, _, b_dlogp, b_stats = GR.loss_bounds(logp, old_logp, ref_logp, adv_seq, seq_off, eps_low, eps_high, beta, loss_type, max_completion_length,
                                            upstream)
    so, lens = GR._lens(seq_off)
    n, R = len(lens), logp.numel()
    lt = GR.LOSS_TYPES.get(loss_type, loss_type)
    if lt == 0:
        w = torch.repeat_interleave(1.0 / (n * torch.tensor(lens, dtype=torch.float64)), torch.tensor(lens))
    else:
        w = torch.full((R,), 1.0 / R if lt == 1 else 1.0 / (n * max_completion_length), dtype=torch.float64)
    dep = GR._fold_depth(math.ceil(R / 64) + math.ceil(n / 16)) * (2 if lt == 0 else 1)
    Habs = torch.zeros(R, dtype=torch.float64) if entropy is None else entropy.double().abs()
    b_stats = dict(b_stats)
    b_stats["loss"] += abs(entropy_coef) * float((w * Habs).sum()) * (2 * dep + 12) * U
    b_stats.update(zero=0.0, entropy=float(Habs.mean()) * (2 * dep + 4) * U, kept_frac=4 * U)
    fails, worst = [], 0.0
    got = got_dlogp.double()
    kept = torch.ones(R, dtype=torch.bool) if keep is None else keep.bool()
    if not bool((got[~kept] == 0).all()):
        fails.append(f"dlogp[{int(((got != 0) & ~kept).nonzero()[0])}]: a masked token carries a gradient")
    err = (got - dlogp).abs()
    zero = dlogp == 0
    if beta == 0 and not bool(((got == 0) == zero).all()):
        fails.append(f"dlogp[{int(((got == 0) != zero).nonzero()[0])}]: the exact zeros are not where autograd's are")
    bad = (err > b_dlogp) & ~(zero & (got == 0))
    ratio = err / b_dlogp.clamp_min(1e-300)
    worst = float(torch.where(zero, torch.zeros_like(ratio), ratio).max())
    if not bool(torch.isfinite(got).all()) or bool(bad.any()):
        i = int((ratio * bad).argmax())
        fails.append(f"dlogp[{i}]: got {float(got[i])!r} want {float(dlogp[i])!r} err/bound {float(ratio[i]):.3g}")
    if got_dent is not None:
        e = (got_dent.double() - dent).abs()
        if not bool((e <= 6 * U * dent.abs()).all()):
            i = int(e.argmax())
            fails.append(f"dent[{i}]: got {float(got_dent[i])!r} want {float(dent[i])!r}")
    for i, name in enumerate(ENT_STAT_NAMES):
        e = abs(float(got_stats[i]) - stats[name])
        worst = max(worst, e / max(b_stats[name], 1e-300)) if b_stats[name] > 0 else worst
        if not e <= b_stats[name]:
            fails.append(f"stat {name}: got {float(got_stats[i])!r} want {stats[name]!r} err {e:.3g} bound {b_stats[name]:.3g}")
    return fails, worst


def replay_grpo_ent(logp, old_logp, ref_logp, adv_seq, seq_off, eps_low, eps_high, beta, loss_type, max_completion_length, upstream, entropy,
                    keep, entropy_coef, fault=None):
    """fp32 restatement of vlr_grpo_loss_ent through autograd -> (dlogp, dent, stats [10]).  fault 'keep_ignored': the mask reaches the
    loss but not dlogp"""
    lp = logp.float().clone().requires_grad_(True)
    Hh = entropy.float().clone().requires_grad_(True)
    f = lambda t: None if t is None else t.float()      # noqa: E731
    total, stats = grpo_ent_loss(lp, f(old_logp), f(ref_logp), adv_seq.float(), seq_off, eps_low, eps_high, beta, loss_type, max_completion_length,
                                 upstream, Hh, keep, entropy_coef)
    total.backward()
    dlogp = lp.grad
    if fault == "keep_ignored":
        lp2 = logp.float().clone().requires_grad_(True)
        grpo_ent_loss(lp2, f(old_logp), f(ref_logp), adv_seq.float(), seq_off, eps_low, eps_high, beta, loss_type, max_completion_length,
                      upstream, entropy.float(), None, entropy_coef)[0].backward()
        dlogp = lp2.grad
    return dlogp, Hh.grad if Hh.grad is not None else torch.zeros_like(dlogp), torch.tensor([stats[k] for k in ENT_STAT_NAMES])


# ------------------------------------------------------------------------------------------------------------ the policy through the oracles
def oracle_heads(W, cfg, pb, emulate=False, lora=None):
    """(token log-probs [R], entropy [R], logits [R][V], seq_off) of the family's oracle forward on the response rows (tests/ppo_ref.py
    policy_heads with the entropy of the same logits: trl's entropy_from_logits)"""
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
    logits = O.lm_logits(hidden[:, :-1][sel], W, emulate, key=key).float()
    lsm = torch.log_softmax(logits, -1)
    tok = lsm.gather(-1, labels[:, 1:][sel].unsqueeze(-1)).squeeze(-1)
    ent = -(torch.exp(lsm) * lsm).sum(-1)
    return tok, ent, logits, [0] + torch.cumsum(sel.sum(-1), 0).tolist()


def high_entropy_mask(ent, q):
    """trl's get_high_entropy_mask on one minibatch's tokens"""
    if q >= 1.0:
        return None
    h = ent.detach().float()
    return h >= torch.quantile(h, 1.0 - q)


def step_grads(W, W_ref, cfg, pb, scores, P, G, hp, minibatches, names, upstream):
    """grpo_ref.step_grads with hp["entropy_coef"] and hp["top_entropy_quantile"]: the mask from the oracle's own entropies, per minibatch
    -> dict(ref, seq_off, advantages, stats [per minibatch, under ENT_STAT_NAMES], keep [per minibatch], entropy [per minibatch], grads)"""
    with torch.no_grad():
        ref_logp, seq_off = GR.token_logps(W_ref, cfg, pb)
    A = GR.advantages(scores.double(), P, G, hp["scale_rewards"])[0].float()
    leaves = {k: W[k].clone().requires_grad_(True) for k in names}
    Wl = dict(W)
    Wl.update(leaves)
    out, keeps, ents = [], [], []
    for rows in minibatches:
        t0, t1 = seq_off[rows[0]], seq_off[rows[-1] + 1]
        so = [x - t0 for x in seq_off[rows[0]:rows[-1] + 2]]
        logp, ent, _, _ = oracle_heads(Wl, cfg, GR._rows(pb, cfg, rows))
        keep = high_entropy_mask(ent, hp["top_entropy_quantile"])
        total, st = grpo_ent_loss(logp, None, ref_logp[t0:t1] if hp["beta"] else None, A[rows], so, hp["epsilon"], hp["epsilon_high"], hp["beta"],
                                  hp["loss_type"], hp.get("max_completion_length", 0), upstream, ent, keep, hp["entropy_coef"])
        total.backward()
        out.append(st), keeps.append(keep), ents.append(ent.detach())
    return dict(ref=ref_logp, seq_off=seq_off, advantages=A, stats=out, keep=keeps, entropy=ents, grads={k: v.grad for k, v in leaves.items()})


def train_steps(W, W_ref, cfg, pb, scores, P, G, hp, steps, num_iterations, mini_batch_size, lr, emulate=False):
    """grpo_ref.train_steps (full fine-tune) with the entropy options -> the per-minibatch stats dicts"""
    from oracle import llava_dpo_oracle as O
    names = GR.full_finetune_names(W)
    master = {k: v.bfloat16().float() for k, v in W.items()}
    rnd = lambda: {k: v.bfloat16().float() for k, v in master.items()}      # noqa: E731
    state, out = {}, []
    N = P * G
    A = GR.advantages(scores.double(), P, G, hp["scale_rewards"])[0].float()
    for _ in range(steps):
        Wp = rnd()
        with torch.no_grad():
            old_logp, seq_off = GR.token_logps(Wp, cfg, pb, emulate)
            ref_logp, _ = GR.token_logps(W_ref, cfg, pb, emulate)
        for _ in range(num_iterations):
            for m0 in range(0, N, mini_batch_size):
                rows = list(range(m0, m0 + mini_batch_size))
                t0, t1 = seq_off[m0], seq_off[m0 + mini_batch_size]
                so = [x - t0 for x in seq_off[m0:m0 + mini_batch_size + 1]]
                leaves = {k: Wp[k].clone().requires_grad_(True) for k in names}
                Wl = dict(Wp)
                Wl.update(leaves)
                logp, ent, _, _ = oracle_heads(Wl, cfg, GR._rows(pb, cfg, rows), emulate)
                keep = high_entropy_mask(ent, hp["top_entropy_quantile"])
                total, st = grpo_ent_loss(logp, old_logp[t0:t1], ref_logp[t0:t1], A[rows], so, hp["epsilon"], hp["epsilon_high"], hp["beta"],
                                          hp["loss_type"], hp.get("max_completion_length", 0), 1.0, ent, keep, hp["entropy_coef"])
                total.backward()
                grads = {k: v.grad for k, v in leaves.items() if v.grad is not None}
                with torch.no_grad():
                    O.adamw_step(master, grads, state, lr, 0.9, 0.999, 1e-8, 0.0)
                Wp = rnd()
                out.append(st)
    return out
