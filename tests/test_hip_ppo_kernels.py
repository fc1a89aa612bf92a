"""vlr_ppo_advantages / vlr_ppo_loss / vlr_v_head_bwd (csrc/ppo.hip) against the fp64 host arithmetic of tests/ppo_ref.py.  Every bound
is derived here from the fp32 unit roundoff u = 2^-24 and the depth of the sum or scan the header documents (thread-strided partials of
ceil(R / 1024) terms, six xor butterflies, sixteen waves in order); none is fitted to the output.  Needs a real MI355X:  pytest -m gpu"""
import math

import pytest
import torch

from tests import ppo_ref as PR

pytestmark = pytest.mark.gpu

from tests.test_hip_e2e import gpu  # noqa: E402,F401

U = 2.0 ** -24
SENTINEL = -7.5


def _depth(R):
    """additions an element passes through in the one-workgroup sums: its thread's stride loop, 6 butterflies, 16 waves"""
    return math.ceil(R / 1024) + 6 + 16


def _mean_bound(absmean, elem_err_mean, R):
    """|fp32 mean - fp64 mean|: the elements' own errors + the summation (2 depth u sum|x|, the _acc_bound of test_hip_rm_kernels.py) + the
    rounding of 1 / R and of the product"""
    return elem_err_mean + (2 * _depth(R) + 4) * U * absmean


def _whiten_err(x, dx, shift_mean):
    """error bound of masked_whiten on fp64 values x known to +-dx -> (per-element bound, bound of the mean, bound of the variance)"""
    R = x.numel()
    m = x.mean()
    v = ((x - m) ** 2).mean() * (R / (R - 1))
    dm = _mean_bound(x.abs().mean(), dx.mean(), R)
    e = dx.max() + dm                                        # error of one centred element
    dv = (2 * v.sqrt() * e + e * e) * (R / (R - 1)) + (2 * _depth(R) + 8) * U * v      # |d var| <= 2 sqrt(var) max|d(x - m)| (Cauchy-Schwarz) + the sum
    y = (x - m) * torch.rsqrt(v + 1e-8)
    dsig = 0.5 * dv / (v + 1e-8) + 3 * U                     # relative error of sqrt(var + eps) and of the division by it
    dy = (dx + dm + U * (x - m).abs()) * torch.rsqrt(v + 1e-8) + y.abs() * (dsig + 2 * U)
    if not shift_mean:
        dy = dy + dm + U * (y + m).abs()
    return dy, dm, dv


# ------------------------------------------------------------------------------------------------------------ vlr_ppo_advantages
ADV_CASES = {
    "n1_two_tokens": [2],
    "n1_past_one_sweep": [1100],
    "n3": [1, 2, 65],
    "n16": [1, 2, 63, 64, 65, 1, 130, 400, 3, 64, 65, 63, 2, 257, 100, 7],
}


def _adv_inputs(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    R, n = sum(lengths), len(lengths)
    seq_off = torch.tensor([0] + torch.tensor(lengths).cumsum(0).tolist(), dtype=torch.int32)
    old = -torch.rand(R, generator=g) * 3
    ref = old + torch.randn(R, generator=g) * 0.3
    values = torch.randn(R, generator=g)
    scores = torch.randn(n, generator=g) * 2
    return old, ref, values, seq_off, scores, R, n


def _run_adv(hip, old, ref, values, seq_off, scores, kl_coef, mode, gamma, lam, whiten, R, n):
    dev = [t.cuda() for t in (old, ref, values, seq_off, scores)]
    adv, ret = torch.full((R + 8,), SENTINEL, device="cuda"), torch.full((R + 8,), SENTINEL, device="cuda")
    kls, stats = torch.full((n + 8,), SENTINEL, device="cuda"), torch.full((12,), SENTINEL, device="cuda")
    hip.call("vlr_ppo_advantages", *dev, kl_coef, PR.KL_MODES[mode], gamma, lam, int(whiten), adv, ret, kls, stats, R, n)
    torch.cuda.synchronize()
    return adv.cpu(), ret.cpu(), kls.cpu(), stats.cpu()


def adv_bounds(old, ref, values, seq_off, scores, kl_coef, mode, gamma, lam, whiten):
    """fp64 replay of vlr_ppo_advantages on fp32 inputs and the derived error bounds of the kernel's outputs
    -> (exp, dict(returns, advantages, mean, var, nsr, kl): per-element bounds of returns and whitened advantages, bounds of the raw
    advantages' mean and variance, and the fp64 non-score rewards and penalties)"""
    exp = PR.advantages(old, ref, values, seq_off, scores, kl_coef, mode, gamma, lam, whiten)
    so = [int(x) for x in seq_off]
    R, n = int(so[-1]), len(so) - 1
    # rewards: d = old - ref (u |d|), the penalty (3 u), * kl_coef (u), + score (u |r|)
    r, nsr, kl = PR.rewards(old.double(), ref.double(), so, scores.double(), kl_coef, mode)
    dr = 5 * U * nsr.abs() + U * r.abs()
    if whiten:
        dr, _, _ = _whiten_err(r, dr, shift_mean=False)
    r = exp["rewards"]
    # the scan: every step rounds delta (3 operations) and A (2), and carries the error of A_{t+1} on with weight gamma lam
    raw, V = exp["raw_advantages"], values.double()
    E = torch.zeros(R, dtype=torch.float64)
    for s in range(n):
        e_next, a_next, v_next = 0.0, 0.0, 0.0
        for t in range(so[s + 1] - 1, so[s] - 1, -1):
            e = float(dr[t]) + 4 * U * (abs(float(r[t])) + gamma * abs(v_next) + abs(float(V[t])) + gamma * lam * abs(a_next) + abs(float(raw[t]))) \
                + gamma * lam * e_next
            E[t], e_next, a_next, v_next = e, e, float(raw[t]), float(V[t])
    b_adv, dm, dv = _whiten_err(raw, E, shift_mean=True)
    return exp, dict(returns=E + U * exp["returns"].abs(), advantages=b_adv, mean=dm, var=dv, nsr=nsr, kl=kl)


@pytest.mark.parametrize("whiten", [False, True])
@pytest.mark.parametrize("mode", ["kl", "abs", "mse"])
@pytest.mark.parametrize("case", sorted(ADV_CASES))
def test_ppo_advantages(gpu, case, mode, whiten):
    from vlrlhf import _hip as hip
    lengths = ADV_CASES[case]
    old, ref, values, seq_off, scores, R, n = _adv_inputs(lengths, seed=len(lengths) * 7 + sum(lengths))
    kl_coef, gamma, lam = 0.2, 0.97, 0.95
    got = _run_adv(hip, old, ref, values, seq_off, scores, kl_coef, mode, gamma, lam, whiten, R, n)
    again = _run_adv(hip, old, ref, values, seq_off, scores, kl_coef, mode, gamma, lam, whiten, R, n)
    for a, b in zip(got, again):
        assert torch.equal(a, b)                                            # fixed reduction order: the same bits from call to call
    adv, ret, kls, stats = got
    for buf, k in ((adv, R), (ret, R), (kls, n), (stats, 4)):
        assert bool((buf[k:] == SENTINEL).all())                            # nothing past the R tokens / n sequences / 4 stats
    exp, bnd = adv_bounds(old, ref, values, seq_off, scores, kl_coef, mode, gamma, lam, whiten)
    so = [int(x) for x in seq_off]
    b_ret, b_adv, dm, dv, nsr, kl = (bnd[k] for k in ("returns", "advantages", "mean", "var", "nsr", "kl"))
    e_ret, e_adv = (ret[:R].double() - exp["returns"]).abs(), (adv[:R].double() - exp["advantages"]).abs()
    print(f"[ppo adv] {case} {mode} whiten={whiten} R={R} worst err/bound returns {float((e_ret / b_ret).max()):.3f} advantages {float((e_adv / b_adv).max()):.3f}")
    assert bool((e_ret <= b_ret).all()), float((e_ret / b_ret).max())
    assert bool((e_adv <= b_adv).all()), float((e_adv / b_adv).max())
    # per-sequence KL sums: lane-strided partials of ceil(L / 64) terms + 6 butterflies
    klabs = torch.stack([kl[so[s]:so[s + 1]].abs().sum() for s in range(n)])
    b_kls = torch.tensor([2 * (math.ceil(L / 64) + 6) + 3 for L in lengths], dtype=torch.float64) * U * klabs
    e_kls = (kls[:n].double() - exp["kl_sums"]).abs()
    assert bool((e_kls <= b_kls).all()), (e_kls, b_kls)
    b_stats = torch.stack([_mean_bound(exp["kl_sums"].abs().mean(), b_kls.mean(), n),
                           2 * R * U * nsr.abs().mean() + 5 * U * nsr.abs().mean(),      # a lane's partial runs over several sequences: at most R terms
                           dm, dv])
    e_stats = (stats[:4].double() - exp["stats"]).abs()
    assert bool((e_stats <= b_stats).all()), (e_stats, b_stats)
    # the whitened advantages have mean 0 and unit (R / (R - 1)) variance
    assert abs(float(adv[:R].double().mean())) <= float(b_adv.mean()) + 1e-12


def test_ppo_advantages_gamma_one_and_zero_kl_coef(gpu):
    """gamma = lam = 1, kl_coef = 0, no whitening of the rewards: the raw advantage of token t is score - V_t, the return is the score"""
    from vlrlhf import _hip as hip
    lengths = [5, 1, 70]
    old, ref, values, seq_off, scores, R, n = _adv_inputs(lengths, seed=11)
    adv, ret, kls, stats = _run_adv(hip, old, ref, values, seq_off, scores, 0.0, "kl", 1.0, 1.0, False, R, n)
    exp_ret = torch.cat([scores[s].expand(L) for s, L in enumerate(lengths)]).double()
    bound = 8 * max(lengths) * U * (exp_ret.abs() + values.double().abs().max())
    assert bool(((ret[:R].double() - exp_ret).abs() <= bound).all())
    assert float(stats[1]) == 0.0                                           # -0 * kl: no non-score reward


# ------------------------------------------------------------------------------------------------------------ vlr_ppo_loss
LOSS_RS = (2, 3, 64, 65, 1025)


def _loss_inputs(R, cr, crv, seed, trip=False):
    """every element is either ON a clip boundary by construction or at least 1e-3 away from one, so that fp32 and fp64 take the same
    branch: ratio = 1 exactly (logp == old), ratios well inside / well outside 1 +- cr on both sides; vpred exactly on V_old +- crv
    (powers of two), well inside and well outside; advantages of both signs"""
    g = torch.Generator().manual_seed(seed)
    kind = torch.arange(R) % 5
    sign = torch.where(torch.rand(R, generator=g) < 0.5, -1.0, 1.0)
    inside = torch.rand(R, generator=g) * max(cr - 0.02, 0.0)               # |ratio - 1| <= cr - 0.02
    outside = cr + 0.05 + torch.rand(R, generator=g) * 0.3
    target = torch.where(kind == 0, torch.ones(R), torch.where(kind <= 2, 1 + sign * inside, 1 + sign * outside))
    old_logp = -torch.rand(R, generator=g) * 3
    logp = torch.where(kind == 0, old_logp, old_logp + torch.log(target))
    if cr == 0.0:                                                           # the bound is exactly 1: leave only exact ones and clear outsiders
        logp = torch.where(kind <= 2, old_logp, logp)
    if trip:
        logp = old_logp + 3.0
    adv = torch.randn(R, generator=g)
    adv = torch.where(adv.abs() < 0.05, torch.full_like(adv, 0.5), adv)
    old_values = torch.where(torch.rand(R, generator=g) < 0.5, 1.0, -2.0)   # powers of two: V_old +- crv is exact for crv = 0.5
    vk = (torch.arange(R) // 5) % 5
    voff = torch.where(vk == 0, torch.full((R,), crv), torch.where(vk == 1, torch.full((R,), -crv),
                       torch.where(vk == 2, (torch.rand(R, generator=g) * 2 - 1) * (crv - 0.02), sign * (crv + 0.05 + torch.rand(R, generator=g)))))
    vpred = old_values + voff
    ret = torch.randn(R, generator=g) * 2
    # max((vpred - ret)^2, (vclip - ret)^2) away from a tie wherever vpred is clipped: ret not within 1e-2 of the midpoint
    vclip = torch.minimum(torch.maximum(vpred, old_values - crv), old_values + crv)
    mid = 0.5 * (vpred + vclip)
    ret = torch.where((vclip != vpred) & ((ret - mid).abs() < 1e-2), ret + 0.5, ret)
    return logp, vpred, old_logp, old_values, adv, ret


def _run_loss(hip, ins, R, cr, crv, vf_coef, thr, upstream):
    dev = [t.cuda() for t in ins]
    dlogp, dvpred = torch.full((R + 8,), SENTINEL, device="cuda"), torch.full((R + 8,), SENTINEL, device="cuda")
    stats = torch.full((24,), SENTINEL, device="cuda")
    hip.call("vlr_ppo_loss", *dev, R, cr, crv, vf_coef, thr, upstream, dlogp, dvpred, stats)
    torch.cuda.synchronize()
    return dlogp.cpu(), dvpred.cpu(), stats.cpu()


@pytest.mark.parametrize("upstream", [1.0, 0.25])
@pytest.mark.parametrize("cr", [0.2, 0.0])
@pytest.mark.parametrize("R", LOSS_RS)
def test_ppo_loss(gpu, R, cr, upstream):
    from vlrlhf import _hip as hip
    crv, vf_coef, thr = 0.5, 0.1, 10.0
    ins = _loss_inputs(R, cr, crv, seed=R + int(cr * 10))
    logp, vpred, old_logp, old_values, adv, ret = (t.double() for t in ins)
    # the construction holds: every ratio / vpred is on a boundary or 1e-3 away from it
    ratio = torch.exp(logp - old_logp)
    for edge in (1 - cr, 1 + cr):
        assert bool(((ratio == edge) | ((ratio - edge).abs() >= 1e-3)).all())
    for edge in (old_values - crv, old_values + crv):
        assert bool(((vpred == edge) | ((vpred - edge).abs() >= 1e-3)).all())
    if R >= 64:
        assert bool((ratio == 1).any()) and bool((ratio > 1 + cr).any()) and bool((ratio < 1 - cr).any())
        assert bool((vpred == old_values + crv).any()) and bool((vpred == old_values - crv).any())
        assert bool((adv > 0).any()) and bool((adv < 0).any())
    got = _run_loss(hip, ins, R, cr, crv, vf_coef, thr, upstream)
    again = _run_loss(hip, ins, R, cr, crv, vf_coef, thr, upstream)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    dlogp, dvpred, stats = got
    assert bool((dlogp[R:] == SENTINEL).all()) and bool((dvpred[R:] == SENTINEL).all()) and bool((stats[17:] == SENTINEL).all())
    exp, e_dlogp, e_dvpred = PR.loss_and_grads(*ins, cr, crv, vf_coef, thr, upstream)
    # per element: d = logp - old (u |d|) through expf (2 ulp): ratio to (|d| + 4) u; the products and the 1 / R, upstream scales on top
    d = (logp - old_logp).abs()
    b_dlogp = (d + 10) * U * e_dlogp.abs()
    err_v = torch.where((vpred - ret).abs() >= (torch.clamp(vpred, old_values - crv, old_values + crv) - ret).abs(), (vpred - ret).abs(),
                        (torch.clamp(vpred, old_values - crv, old_values + crv) - ret).abs())
    vmag = old_values.abs() + crv + ret.abs() + vpred.abs()
    gv = upstream * vf_coef * 0.5 / R
    b_dvpred = gv * 2 * U * vmag + 6 * U * e_dvpred.abs()
    el, ev = (dlogp[:R].double() - e_dlogp).abs(), (dvpred[:R].double() - e_dvpred).abs()
    print(f"[ppo loss] R={R} cr={cr} up={upstream} worst err/bound dlogp {float((el / b_dlogp.clamp_min(1e-300)).max()):.3f} "
          f"dvpred {float((ev / b_dvpred.clamp_min(1e-300)).max()):.3f}")
    assert bool((el <= b_dlogp).all()), float((el / b_dlogp.clamp_min(1e-300)).max())
    assert bool((ev <= b_dvpred).all()), float((ev / b_dvpred.clamp_min(1e-300)).max())
    assert bool(((dlogp[:R] == 0) == (e_dlogp == 0)).all()) and bool(((dvpred[:R] == 0) == (e_dvpred == 0)).all())      # clipped elements: exactly 0
    # stats: element errors + the sums
    pg_el = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - cr, 1 + cr))
    vf_el = err_v ** 2
    b_pg = _mean_bound(pg_el.abs().mean(), ((d + 6) * U * pg_el.abs()).mean(), R)
    b_vf = 0.5 * _mean_bound(vf_el.mean(), (2 * err_v * U * vmag + 3 * U * vf_el).mean(), R) + U * abs(exp["vf"])
    dm_ret, dv_ret = _whiten_err(ret, torch.zeros(R, dtype=torch.float64), True)[1:]
    dm_vp, dv_vp = _whiten_err(vpred, torch.zeros(R, dtype=torch.float64), True)[1:]
    dm_ov, dv_ov = _whiten_err(old_values, torch.zeros(R, dtype=torch.float64), True)[1:]
    bounds = dict(loss=b_pg + vf_coef * b_vf + 3 * U * (abs(exp["pg"]) + vf_coef * abs(exp["vf"])), pg=b_pg, vf=b_vf,
                  approxkl=0.5 * _mean_bound((d * d).mean(), (3 * U * d * d).mean(), R) + U * exp["approxkl"],
                  policykl=_mean_bound(d.mean(), (U * d).mean(), R), pg_clipfrac=4 * U, vf_clipfrac=4 * U,
                  ratio=_mean_bound(ratio.mean(), ((d + 4) * U * ratio).mean(), R), returns_mean=dm_ret, returns_var=dv_ret,
                  vpred_mean=dm_vp, vpred_var=dv_vp, error=_mean_bound(((vpred - ret) ** 2).mean(), (3 * U * (vpred - ret) ** 2).mean(), R),
                  advantages_mean=_mean_bound(adv.abs().mean(), 0.0, R), values_mean=dm_ov, values_var=dv_ov, skipped=0.0)
    for i, name in enumerate(PR.STAT_NAMES):
        err = abs(float(stats[i]) - exp[name])
        assert err <= float(bounds[name]), (name, float(stats[i]), exp[name], err, float(bounds[name]))
    assert exp["skipped"] == 0.0


@pytest.mark.parametrize("R", (3, 1025))
def test_ppo_loss_ratio_threshold_zeroes_everything(gpu, R):
    from vlrlhf import _hip as hip
    ins = _loss_inputs(R, 0.2, 0.5, seed=R, trip=True)                       # ratio = e^3 everywhere > the threshold 10
    dlogp, dvpred, stats = _run_loss(hip, ins, R, 0.2, 0.5, 0.1, 10.0, 1.0)
    assert float(stats[7]) > 10.0 and float(stats[16]) == 1.0
    assert float(stats[0]) == 0.0 and float(stats[1]) == 0.0 and float(stats[2]) == 0.0
    assert bool((dlogp[:R] == 0).all()) and bool((dvpred[:R] == 0).all())
    assert bool((dlogp[R:] == SENTINEL).all()) and bool((dvpred[R:] == SENTINEL).all())
    exp, e_dlogp, e_dvpred = PR.loss_and_grads(*ins, 0.2, 0.5, 0.1, 10.0)
    assert exp["skipped"] == 1.0 and exp["loss"] == 0.0 and float(e_dlogp.abs().sum()) == 0.0 and float(e_dvpred.abs().sum()) == 0.0
    assert abs(float(stats[12]) - exp["error"]) <= _mean_bound(exp["error"], 3 * U * exp["error"], R)      # the other stats are still reported
    # just under the threshold nothing is zeroed
    dlogp, dvpred, stats = _run_loss(hip, ins, R, 0.2, 0.5, 0.1, 25.0, 1.0)
    assert float(stats[16]) == 0.0 and float(stats[0]) != 0.0 and bool((dvpred[:R] != 0).any())


# ------------------------------------------------------------------------------------------------------------ vlr_v_head_bwd
HS = (8, 136, 2056, 4096)          # one 16-byte group; not a multiple of the 64-lane wave; past 32 and 64 column groups with a remainder; the 7B width
RS = (1, 3, 64, 65, 300)           # one row; inside one chunk of 8; whole chunks; a chunk of one row; more than 8 chunks per fold strand
PAD = 5                            # sentinel rows behind the R rows


def _vh_depth(R):
    """additions on the way of a d w element: the rows of its chunk, the chunks of its fold strand, the 8 strands, the old gradient"""
    rc = max(8, math.ceil(R / 256))
    return rc + math.ceil(math.ceil(R / rc) / 8) + 8 + 1


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("R", RS)
def test_v_head_bwd(gpu, H, R):
    from vlrlhf import _hip as hip
    g = torch.Generator().manual_seed(5 * H + R)
    hg = torch.randn(R + PAD, H, generator=g).bfloat16()
    w = ((torch.rand(H, generator=g) * 2 - 1) / H ** 0.5).bfloat16()
    gr = torch.randn(R, generator=g)
    dhg0 = torch.randn(R, H, generator=g).bfloat16()
    old_w = torch.randn(H, generator=torch.Generator().manual_seed(1)).bfloat16()
    old_b = torch.tensor([0.75]).bfloat16()
    ws_bytes = hip.lib().vlr_v_head_bwd_workspace_bytes(R, H)
    rc = max(8, math.ceil(R / 256))
    assert ws_bytes == math.ceil(R / rc) * (H + 1) * 4
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    x = hg[:R].double()
    absdw, absdb = gr.double().abs() @ x.abs(), gr.double().abs().sum()
    outs = []
    for acc in (0, 1, 1):
        dhg = torch.cat([dhg0, torch.full((PAD, H), SENTINEL).bfloat16()]).cuda()
        dw, db = old_w.clone().cuda(), torch.cat([old_b, torch.full((7,), SENTINEL).bfloat16()]).cuda()
        hip.call("vlr_v_head_bwd", hg.cuda(), w.cuda(), gr.cuda(), dhg, dw, db, acc, ws, R, H)
        torch.cuda.synchronize()
        dhg, dw, db = dhg.cpu(), dw.cpu(), db.cpu()
        outs.append((dhg, dw, db))
        e_dhg, e_dw, e_db = PR.v_head_bwd(x, w, gr, dhg0, old_w if acc else None, old_b if acc else None)
        e_bf = e_dhg.float().bfloat16().double()                           # the fp64 sum rounded to bf16
        assert bool(((dhg[:R].double() - e_bf).abs() <= 2.0 ** -7 * e_bf.abs()).all())      # one bf16 ulp (2^-7 |x| is at least the spacing at x)
        assert bool((dhg[R:].float() == SENTINEL).all())                   # rows beyond R untouched
        # one bf16 rounding (unit roundoff 2^-8) of the fp64 value + the fp32 accumulation along the documented order
        bw = 2.0 ** -8 * e_dw.abs() + 2 * _vh_depth(R) * U * (absdw + old_w.double().abs() * acc)
        bb = 2.0 ** -8 * e_db.abs() + 2 * (_vh_depth(R) + 22) * U * (absdb + old_b.double().abs() * acc)
        ew, eb = (dw.double() - e_dw).abs(), (db[:1].double() - e_db).abs()
        print(f"[v_head bwd] H={H} R={R} acc={acc} worst dw err/bound {float((ew / bw.clamp_min(1e-30)).max()):.3f} db {float(eb / bb):.3f}")
        assert bool((ew <= bw).all()) and bool((eb <= bb).all()), (acc, float(ew.max()), float(eb))
        assert bool((db[1:].float() == SENTINEL).all())                    # the bias gradient is ONE element
    for a, b in zip(outs[1], outs[2]):
        assert torch.equal(a, b)                                           # fixed fold order: the same bits from call to call


def test_v_head_bwd_zero_gradient_leaves_dhg(gpu):
    from vlrlhf import _hip as hip
    R, H = 65, 136
    g = torch.Generator().manual_seed(3)
    hg, w = torch.randn(R, H, generator=g).bfloat16().cuda(), torch.randn(H, generator=g).bfloat16().cuda()
    dhg0 = torch.randn(R, H, generator=g).bfloat16()
    dhg, dw, db = dhg0.clone().cuda(), torch.ones(H).bfloat16().cuda(), torch.ones(8).bfloat16().cuda()
    ws = torch.empty(hip.lib().vlr_v_head_bwd_workspace_bytes(R, H), dtype=torch.uint8, device="cuda")
    hip.call("vlr_v_head_bwd", hg, w, torch.zeros(R, device="cuda"), dhg, dw, db, 0, ws, R, H)
    torch.cuda.synchronize()
    assert torch.equal(dhg.cpu(), dhg0) and float(dw.float().abs().sum()) == 0.0 and float(db[0]) == 0.0
