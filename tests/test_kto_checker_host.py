"""The KTO checker checked (CPU): tests/kto_ref.py on hand-computed cases, its closed form against torch autograd of the one-expression
loss, a numpy fp32 stand-in for vlr_kto_loss that it accepts, and planted faults in that stand-in's output that it must reject - each
fault is one way of getting trl's KTOTrainer.kto_loss wrong."""
import math

import numpy as np
import pytest
import torch

from tests import kto_ref as KR

BETA, W_D, W_U, UP = 0.1, 1.25, 0.75, 0.5


def standin(pi, ref, label, pi_kl, ref_kl, beta, w_d, w_u, upstream, *, clamp=True, kl_grad=False, flip_undesirable=False, swap_weights=False,
            class_mean=False, drop_upstream=False):
    """vlr_kto_loss in numpy fp32, statement by statement (sums in numpy's order, not the kernel's: the bounds cover any order of that
    depth) -> (losses, rewards, dpi, stats [8]); every keyword plants one fault"""
    f = np.float32
    pi, ref, pi_kl, ref_kl = (np.asarray(t, dtype=f) for t in (pi, ref, pi_kl, ref_kl))
    lab = np.asarray(label) != 0
    n, m = pi.size, pi_kl.size
    beta, w_d, w_u, upstream = f(beta), f(w_d), f(w_u), f(upstream)
    if swap_weights:
        w_d, w_u = w_u, w_d
    kl = f((pi_kl - ref_kl).sum(dtype=f) / f(m))
    if clamp:
        kl = max(kl, f(0))
    r = pi - ref
    z = np.where(lab, beta * (r - kl), beta * (kl - r)).astype(f)
    if flip_undesirable:
        z = np.where(lab, z, -z).astype(f)
    with np.errstate(over="ignore"):
        q = (f(1) / (f(1) + np.exp(z, dtype=f))).astype(f)
    w = np.where(lab, w_d, w_u).astype(f)
    losses = w * q
    rewards = beta * r
    nd = f(lab.sum())
    div = np.where(lab, nd, f(n) - nd).astype(f) if class_mean else np.full(n, n, dtype=f)
    c = w * beta / div * (f(1) if drop_upstream else upstream)
    g0 = q * (f(1) - q)
    dpi = np.where(lab, -c, c).astype(f) * g0
    if kl_grad:      # kl treated as a function of the batch's own rows: every row gets a share of d loss / d kl
        dkl = (np.where(lab, c, -c).astype(f) * g0).sum(dtype=f)
        dpi = dpi + dkl / f(n)
    loss = (losses / div).sum(dtype=f) if class_mean else losses.sum(dtype=f) / f(n)
    stats = np.array([loss, kl, rewards[lab].sum(dtype=f), rewards[~lab].sum(dtype=f), pi[lab].sum(dtype=f), pi[~lab].sum(dtype=f), nd, f(n) - nd],
                     dtype=f)
    return losses, rewards, dpi, stats


def _check(out, inputs, up=UP):
    return KR.check(*out, *inputs, BETA, W_D, W_U, up)


# ------------------------------------------------------------------------------------------------------------ the checker, by hand
def test_replay_by_hand():
    ln3 = math.log(3.0)
    # kl = max(0, mean(1, 3)) = 2; beta = 1: row 0 desirable r = 2 + ln 3 -> s = 3/4; row 1 undesirable r = 2 + ln 3 -> s = 1/4; row 2 desirable r = 2
    pi = torch.tensor([2 + ln3, 2 + ln3, 2.0], dtype=torch.float64)
    rp = KR.replay(pi, torch.zeros(3).double(), [1, 0, 1], torch.tensor([1.0, 3.0]).double(), torch.zeros(2).double(), 1.0, 2.0, 4.0, 0.5)
    assert rp["kl"] == 2.0
    assert torch.allclose(rp["losses"], torch.tensor([2 * 0.25, 4 * 0.75, 2 * 0.5], dtype=torch.float64), rtol=0, atol=1e-14)
    assert torch.allclose(rp["dpi"], torch.tensor([-(2 / 3) * 3 / 16, (4 / 3) * 3 / 16, -(2 / 3) / 4], dtype=torch.float64) * 0.5, rtol=0, atol=1e-14)
    assert torch.allclose(rp["rewards"], pi, rtol=0, atol=0)
    want = [(0.5 + 3.0 + 1.0) / 3, 2.0, 4 + ln3, 2 + ln3, 4 + ln3, 2 + ln3, 2.0, 1.0]
    assert torch.allclose(rp["stats"], torch.tensor(want, dtype=torch.float64), rtol=0, atol=1e-13)
    # a negative mean on the KL rows: kl is 0, not the mean
    rp = KR.replay(pi, torch.zeros(3).double(), [1, 0, 1], torch.tensor([-1.0, -3.0]).double(), torch.zeros(2).double(), 1.0, 2.0, 4.0)
    assert rp["kl"] == 0.0 and float(rp["stats"][1]) == 0.0


@pytest.mark.parametrize("labels", ["ones", "zeros", "mixed"])
@pytest.mark.parametrize("kl_mean", [1.5, -2.0])
def test_closed_form_is_autograd_of_the_one_expression(labels, kl_mean):
    """the gradient of the header is torch autograd's of the loss written as ONE expression with the KL baseline detached"""
    inp = KR.make_inputs(40, 7, labels, BETA, kl_mean, seed=3)
    pi = inp[0].double().clone().requires_grad_(True)
    f32 = KR._f32      # the replay rounds the four scalars to fp32 as the C ABI does: hand the expression the same values
    total, kl, losses, rewards = KR.loss(pi, inp[1].double(), inp[2], inp[3].double(), inp[4].double(), f32(BETA), f32(W_D), f32(W_U), f32(UP))
    total.backward()
    rp = KR.replay(*inp, BETA, W_D, W_U, UP)
    # (autograd forms 1 - sigmoid with a cancellation the replay avoids: an absolute 2^-52 of the weight w beta upstream / n < 2e-3)
    assert torch.allclose(pi.grad, rp["dpi"], rtol=1e-9, atol=2e-3 * 2.0 ** -52) and abs(float(kl) - rp["kl"]) < 1e-12
    assert torch.allclose(losses.detach(), rp["losses"], rtol=1e-9, atol=2 * 2.0 ** -52) and torch.allclose(rewards.detach(), rp["rewards"], rtol=1e-12, atol=0)
    assert (kl_mean < 0) == (rp["kl"] == 0.0)


# ------------------------------------------------------------------------------------------------------------ accepted, and every fault rejected
CASES = [(65, 64, "mixed", 1.5), (1025, 65, "mixed", 1.5), (64, 1, "mixed", -2.0), (63, 64, "ones", 0.7), (63, 64, "zeros", 0.7)]


@pytest.mark.parametrize("n,m,labels,kl_mean", CASES)
def test_checker_accepts_the_fp32_standin(n, m, labels, kl_mean):
    inp = KR.make_inputs(n, m, labels, BETA, kl_mean, seed=n + m)
    cnt = KR.branch_counts(*inp, BETA)
    assert sum(cnt.values()) == n
    fails, worst = _check(standin(*inp, BETA, W_D, W_U, UP), inp)
    assert fails == [] and worst <= 1.0, (fails, worst)


FAULTS = {
    "kl not clamped at 0": (dict(clamp=False), -2.0),
    "a gradient flowing through kl": (dict(kl_grad=True), 1.5),
    "the sign of the undesirable branch": (dict(flip_undesirable=True), 1.5),
    "weights swapped": (dict(swap_weights=True), 1.5),
    "mean over the labelled class only": (dict(class_mean=True), 1.5),
    "upstream dropped": (dict(drop_upstream=True), 1.5),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_checker_rejects_planted_fault(fault):
    kw, kl_mean = FAULTS[fault]
    inp = KR.make_inputs(65, 64, "mixed", BETA, kl_mean, seed=11)
    assert _check(standin(*inp, BETA, W_D, W_U, UP), inp)[0] == []          # the same inputs without the fault pass
    fails, _ = _check(standin(*inp, BETA, W_D, W_U, UP, **kw), inp)
    assert fails, f"{fault}: not flagged"


def test_checker_rejects_nan_inexact_saturation_and_wrong_counts():
    inp = KR.make_inputs(65, 64, "mixed", BETA, 1.5, seed=11)
    good = standin(*inp, BETA, W_D, W_U, UP)
    rp = KR.replay(*inp, BETA, W_D, W_U, UP)
    sat = int((rp["z"] > KR.SAT_HI).nonzero()[0])
    for slot, val in ((2, np.nan), (2, 1e-30), (0, 1e-30)):      # dpi NaN; a saturated row whose gradient / loss is tiny but not 0
        out = [np.array(t, copy=True) for t in good]
        out[slot][sat] = val
        assert _check(out, inp)[0], (slot, val)
    out = [np.array(t, copy=True) for t in good]
    out[3][6] += 1
    out[3][7] -= 1
    assert any("count" in f for f in _check(out, inp)[0])
