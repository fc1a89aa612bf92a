"""The checker of the GRPO kernel tests (tests/grpo_ref.py check_advantages / check_loss) on the CPU: it passes the fp64 reference rounded
to fp32 - what a correct kernel may return - and flags each of the faults planted here, one at a time: a tie that is not halved, a
gradient on the clipped side, the sequence mean traded for the token mean, the biased std, a sequence boundary off by one, the KL
gradient with the wrong sign."""
import pytest
import torch

from tests import grpo_ref as GR

EPS, BETA = 0.2, 0.04


def _inputs(seed=0, lengths=(40, 1, 70, 9, 30)):
    """ratios on every branch (tests/grpo_ref.py branch_inputs); advantages of both signs and a zero"""
    return GR.branch_inputs(list(lengths), [1.5, -0.75, -1.25, 0.0, 2.0], EPS, EPS, seed)


def _as_kernel(stats, dlogp):
    """the fp64 reference the way a correct kernel returns it: fp32, the stats in the kernel's order"""
    return dlogp.float(), torch.tensor([stats[k] for k in GR.STAT_NAMES] + [0.0], dtype=torch.float32)


@pytest.mark.parametrize("beta", [0.0, BETA])
@pytest.mark.parametrize("loss_type", ["grpo", "bnpo", "dr_grpo"])
def test_checker_passes_the_reference_itself(loss_type, beta):
    logp, old, ref, adv, so = _inputs()
    cnt = GR.branch_counts(logp, old, adv, so, EPS, EPS)
    assert all(cnt[b] >= 8 for b in GR.BRANCHES), cnt
    for up in (1.0, 0.25):
        st, dl = GR.loss_and_grad(logp, old, ref, adv, so, EPS, EPS, beta, loss_type, 64, up)
        fails, worst = GR.check_loss(*_as_kernel(st, dl), logp, old, ref if beta else None, adv, so, EPS, EPS, beta, loss_type, 64, up)
        assert fails == [] and worst <= 1.0, (fails, worst)


@pytest.mark.parametrize("scale", [True, False])
def test_checker_passes_the_reference_advantages(scale):
    g = torch.Generator().manual_seed(1)
    P, G = 5, 7
    s = torch.randn(P * G, generator=g)
    s[2 * G:3 * G] = 0.1                                      # a group of equal scores
    A, st = GR.advantages(s.double(), P, G, scale)
    fails, worst = GR.check_advantages(A.float(), torch.cat([st, torch.zeros(1).double()]).float(), s, P, G, scale)
    assert fails == [] and worst <= 1.0, (fails, worst)
    # a NaN in the equal group, or a wrong count of such groups, is named
    bad = A.float().clone()
    bad[2 * G] = float("nan")
    assert any("equal scores" in f or "finite" in f for f in GR.check_advantages(bad, st.float(), s, P, G, scale)[0])
    st2 = st.float().clone()
    st2[2] = 0.0
    assert any("frac_reward_zero_std" in f for f in GR.check_advantages(A.float(), st2, s, P, G, scale)[0])


def _flags(dl, st, loss_type="grpo", beta=BETA):
    logp, old, ref, adv, so0 = _inputs()
    return GR.check_loss(*_as_kernel(st, dl), logp, old, ref if beta else None, adv, so0, EPS, EPS, beta, loss_type, 64)[0]


def test_checker_flags_a_tie_that_is_not_halved():
    """inside the range both branches of min() are equal: a kernel that hands the tie's gradient to ONE branch at half weight returns
    0.5 A r there"""
    logp, old, ref, adv, so = _inputs()
    st, dl = GR.loss_and_grad(logp, old, ref, adv, so, EPS, EPS, 0.0, "grpo", 64)
    r = torch.exp(logp.double() - old.double())
    inside = (r >= 1 - EPS) & (r <= 1 + EPS)
    fails = _flags(torch.where(inside, 0.5 * dl, dl), st, beta=0.0)
    assert fails and all(f.startswith("dlogp") for f in fails)


def test_checker_flags_a_gradient_on_the_clipped_side():
    logp, old, ref, adv, so = _inputs()
    for beta in (0.0, BETA):
        st, dl = GR.loss_and_grad(logp, old, ref, adv, so, EPS, EPS, beta, "bnpo", 64)
        _, unclipped = GR.loss_and_grad(logp, old, ref, adv, so, 1e9, 1e9, beta, "bnpo", 64)      # no clipping at all: -A r everywhere
        assert bool((unclipped != dl).any())
        fails = _flags(unclipped, st, "bnpo", beta)
        assert fails and all(f.startswith("dlogp") for f in fails)


def test_checker_flags_sequence_mean_traded_for_token_mean():
    logp, old, ref, adv, so = _inputs()
    st, dl = GR.loss_and_grad(logp, old, ref, adv, so, EPS, EPS, BETA, "bnpo", 64)
    fails = _flags(dl, st, "grpo")
    assert any(f.startswith("stat loss") for f in fails) and any(f.startswith("dlogp") for f in fails)
    st, dl = GR.loss_and_grad(logp, old, ref, adv, so, EPS, EPS, BETA, "grpo", 64)
    assert any(f.startswith("stat loss") for f in _flags(dl, st, "bnpo"))
    assert any(f.startswith("stat loss") for f in _flags(dl, st, "dr_grpo"))


def test_checker_flags_the_biased_std():
    g = torch.Generator().manual_seed(2)
    for G in (2, 3, 64):
        P = 4
        s = torch.randn(P * G, generator=g)
        A, st = GR.advantages(s.double(), P, G, True)
        x = s.double().reshape(P, G)
        biased = x.std(1, unbiased=False, keepdim=True)
        wrong = ((x - x.mean(1, keepdim=True)) / (biased + 1e-4)).reshape(-1)
        fails, _ = GR.check_advantages(wrong.float(), st.float(), s, P, G, True)
        assert any(f.startswith("advantages[") for f in fails), G
        st2 = st.clone()
        st2[1] = biased.mean()
        assert any("reward_std" in f for f in GR.check_advantages(A.float(), st2.float(), s, P, G, True)[0]), G


def test_checker_flags_a_sequence_boundary_off_by_one():
    logp, old, ref, adv, so = _inputs()
    for s in range(1, len(so) - 1):
        for step in (-1, 1):
            moved = list(so)
            moved[s] += step
            if not moved[s - 1] < moved[s] < moved[s + 1]:
                continue
            st, dl = GR.loss_and_grad(logp, old, ref, adv, moved, EPS, EPS, BETA, "grpo", 64)
            assert _flags(dl, st), (s, step)


def test_checker_flags_the_kl_gradient_with_the_wrong_sign():
    logp, old, ref, adv, so = _inputs()
    st, dl = GR.loss_and_grad(logp, old, ref, adv, so, EPS, EPS, BETA, "grpo", 64)
    _, dl0 = GR.loss_and_grad(logp, old, ref, adv, so, EPS, EPS, 0.0, "grpo", 64)
    fails = _flags(dl0 - (dl - dl0), st)                      # the policy part + the KL part negated
    assert fails and all(f.startswith("dlogp") for f in fails)
