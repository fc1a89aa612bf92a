"""vlr_grpo_advantages / vlr_grpo_loss (csrc/grpo.hip) against the fp64 host arithmetic of tests/grpo_ref.py at the edges of their loops.
The one comparison is grpo_ref.check_advantages / check_loss, whose bounds are formulas of the fp32 unit roundoff, the depth of the sums
the header documents (lane-strided partials, six xor butterflies, sixteen waves in order), the magnitude of the terms and expf's 2 ulp;
tests/test_grpo_checker_host.py shows that it flags planted faults.  Needs a real MI355X:  pytest -m gpu"""
import pytest
import torch

from tests import grpo_ref as GR

pytestmark = pytest.mark.gpu

from tests.test_hip_e2e import gpu  # noqa: E402,F401

SENTINEL = -7.5
WAVES = 16                                                     # the one workgroup of both kernels: 1024 threads


# ------------------------------------------------------------------------------------------------------------ vlr_grpo_advantages
def _run_adv(hip, scores, P, G, scale):
    adv = torch.full((P * G + 8,), SENTINEL, device="cuda")
    stats = torch.full((12,), SENTINEL, device="cuda")
    hip.call("vlr_grpo_advantages", scores.cuda(), P, G, int(scale), adv, stats)
    torch.cuda.synchronize()
    return adv.cpu(), stats.cpu()


@pytest.mark.parametrize("scale", [True, False])
@pytest.mark.parametrize("P", [1, WAVES, WAVES + 1, 2 * WAVES + 3])      # one group; a group per wave; a wave with a second group; a ragged third round
@pytest.mark.parametrize("G", [2, 3, 64, 65])                 # the smallest group; an odd one; one sweep of the lanes; one element into the second
def test_grpo_advantages(gpu, G, P, scale):
    from vlrlhf import _hip as hip
    g = torch.Generator().manual_seed(100 * G + P)
    s = torch.randn(P * G, generator=g) * 2 + 0.5
    if P >= 2:
        s[(P - 1) * G:] = 0.1                                 # the last group: equal scores whose fp32 mean is not 0.1
    if P >= 3:
        s[G:2 * G] = s[G]                                     # and one more, so that the fraction is not 1 / P
    got = _run_adv(hip, s, P, G, scale)
    again = _run_adv(hip, s, P, G, scale)
    assert all(torch.equal(a, b) for a, b in zip(got, again))                 # fixed reduction order: the same bits from call to call
    adv, stats = got
    assert bool((adv[P * G:] == SENTINEL).all()) and bool((stats[4:] == SENTINEL).all()) and float(stats[3]) == 0.0
    fails, worst = GR.check_advantages(adv[:P * G], stats[:4], s, P, G, scale)
    print(f"[grpo adv] P={P} G={G} scale={scale} worst err/bound {worst:.3f}")
    assert fails == [], fails
    if P >= 2:
        assert bool((adv[(P - 1) * G:P * G] == 0).all())      # A == 0 exactly, never NaN
        assert float(stats[2]) == float(torch.tensor(2.0 if P >= 3 else 1.0) / torch.tensor(float(P)))      # the fraction is exact


def test_grpo_advantages_all_groups_equal_and_huge_offset(gpu):
    """every group equal: all zeros, std stat 0, fraction 1; and scores far from 0 whose differences are small - the shifted moments keep
    them (the bounds are in the differences, not in the offset)"""
    from vlrlhf import _hip as hip
    P, G = 3, 5
    s = torch.tensor([0.3, -1.7, 1e6]).repeat_interleave(G)
    adv, stats = _run_adv(hip, s, P, G, True)
    assert bool((adv[:P * G] == 0).all()) and float(stats[1]) == 0.0 and float(stats[2]) == 1.0
    s = 4096.0 + torch.arange(P * G, dtype=torch.float32) * 0.25            # exact in fp32
    adv, stats = _run_adv(hip, s, P, G, True)
    fails, _ = GR.check_advantages(adv[:P * G], stats[:4], s, P, G, True)
    assert fails == [], fails


# ------------------------------------------------------------------------------------------------------------ vlr_grpo_loss
EPS_LOW, EPS_HIGH, BETA, MCL = 0.2, 0.28, 0.04, 48
ADV_CYCLE = [1.5, -0.75, -1.25, 0.0, 2.0]
LOSS_CASES = {
    "R1": [1],                                                 # one token, n == R
    "n_eq_R_past_the_waves": [1] * (WAVES + 1),               # every sequence one token; n one above the wave count
    "one_token_among_long": [130, 1, 200],
    "lanes_minus_1": [63], "lanes": [64], "lanes_plus_1": [65],              # a sequence at, one below and one above the wave's stride
    "threads_minus_1": [1023], "threads": [1024], "threads_plus_1": [1025],  # R at, one below and one above the workgroup's thread count
    "branches": [40, 1, 70, 9, 30, 2, 64, 65, 3, 17, 128, 5, 33, 1, 90, 7, 66],      # n = 17, every branch at least 8 times
}


def _run_loss(hip, logp, old, ref, adv, so, beta, lt, up, eps=(EPS_LOW, EPS_HIGH)):
    R, n = logp.numel(), len(so) - 1
    dev = lambda t: None if t is None else t.cuda()            # noqa: E731
    dlogp = torch.full((R + 8,), SENTINEL, device="cuda")
    stats = torch.full((16,), SENTINEL, device="cuda")
    hip.call("vlr_grpo_loss", logp.cuda(), dev(old), dev(ref), adv.cuda(), torch.tensor(so, dtype=torch.int32).cuda(), R, n, eps[0], eps[1],
             beta, GR.LOSS_TYPES[lt], MCL, up, dlogp, stats)
    torch.cuda.synchronize()
    return dlogp.cpu(), stats.cpu()


@pytest.mark.parametrize("up", [1.0, 0.25])
@pytest.mark.parametrize("beta", [0.0, BETA])
@pytest.mark.parametrize("lt", sorted(GR.LOSS_TYPES))
@pytest.mark.parametrize("case", sorted(LOSS_CASES))
def test_grpo_loss(gpu, case, lt, beta, up):
    from vlrlhf import _hip as hip
    lengths = LOSS_CASES[case]
    logp, old, ref, adv, so = GR.branch_inputs(lengths, ADV_CYCLE, EPS_LOW, EPS_HIGH, seed=sum(lengths) + len(lengths))
    R = sum(lengths)
    # the construction holds in fp64: every ratio is exactly 1 or at least 1e-3 away from both bounds
    r = torch.exp(logp.double() - old.double())
    for edge in (1 - EPS_LOW, 1 + EPS_HIGH):
        assert bool(((r == 1) | ((r - edge).abs() >= 1e-3)).all())
    cnt = GR.branch_counts(logp, old, adv, so, EPS_LOW, EPS_HIGH)
    assert sum(cnt.values()) == R
    if case == "branches":
        assert all(cnt[b] >= 8 for b in GR.BRANCHES), cnt                     # no branch is tested on a handful of tokens
    got = _run_loss(hip, logp, old, ref if beta else None, adv, so, beta, lt, up)
    again = _run_loss(hip, logp, old, ref if beta else None, adv, so, beta, lt, up)
    assert all(torch.equal(a, b) for a, b in zip(got, again))                 # fixed reduction order: the same bits from call to call
    dlogp, stats = got
    assert bool((dlogp[R:] == SENTINEL).all()) and bool((stats[8:] == SENTINEL).all()) and float(stats[7]) == 0.0
    fails, worst = GR.check_loss(dlogp[:R], stats[:8], logp, old, ref if beta else None, adv, so, EPS_LOW, EPS_HIGH, beta, lt, MCL, up)
    print(f"[grpo loss] {case} {lt} beta={beta} up={up} R={R} n={len(lengths)} branches {cnt} worst err/bound {worst:.3f}")
    assert fails == [], fails
    if beta == 0:
        assert float(stats[1]) == 0.0                         # no KL term: its mean is exactly 0
        with_ref = _run_loss(hip, logp, old, ref, adv, so, 0.0, lt, up)       # beta = 0 never reads the reference: the same bits with one
        assert all(torch.equal(a, b) for a, b in zip(got, with_ref))


@pytest.mark.parametrize("beta", [0.0, BETA])
@pytest.mark.parametrize("lt", sorted(GR.LOSS_TYPES))
def test_grpo_loss_null_old_logp_is_a_copy_of_logp(gpu, lt, beta):
    """old_logp = NULL stands for logp itself: the bits of old_logp = a copy of logp; the ratio is exactly 1, nothing is clipped and the
    gradient still flows"""
    from vlrlhf import _hip as hip
    lengths = LOSS_CASES["branches"]
    logp, _, ref, adv, so = GR.branch_inputs(lengths, ADV_CYCLE, EPS_LOW, EPS_HIGH, seed=5)
    R = sum(lengths)
    null = _run_loss(hip, logp, None, ref if beta else None, adv, so, beta, lt, 0.5)
    copy = _run_loss(hip, logp, logp.clone(), ref if beta else None, adv, so, beta, lt, 0.5)
    assert all(torch.equal(a, b) for a, b in zip(null, copy))
    dlogp, stats = null
    assert float(stats[5]) == 1.0 and float(stats[2]) == 0.0 and float(stats[3]) == 0.0 and float(stats[4]) == 0.0
    fails, _ = GR.check_loss(dlogp[:R], stats[:8], logp, None, ref if beta else None, adv, so, EPS_LOW, EPS_HIGH, beta, lt, MCL, 0.5)
    assert fails == [], fails
    A = torch.repeat_interleave(adv, torch.tensor(lengths))
    if beta == 0:
        assert bool(((dlogp[:R] == 0) == (A == 0)).all()) and bool((dlogp[:R][A > 0] < 0).all()) and bool((dlogp[:R][A < 0] > 0).all())


@pytest.mark.parametrize("lt", sorted(GR.LOSS_TYPES))
def test_grpo_loss_zero_eps_ratio_on_both_bounds(gpu, lt):
    """eps_low = eps_high = 0 with old_logp = NULL: the ratio equals both bounds exactly; the closed interval passes the gradient and the
    halved tie adds two equal halves: d l / d logp = -A, times the weight"""
    from vlrlhf import _hip as hip
    lengths = [5, 1, 70]
    logp, _, _, adv, so = GR.branch_inputs(lengths, [1.5, -0.75, 2.0], 0.0, 0.0, seed=9)
    R, n = sum(lengths), len(lengths)
    dlogp, stats = _run_loss(hip, logp, None, None, adv, so, 0.0, lt, 1.0, eps=(0.0, 0.0))
    assert float(stats[5]) == 1.0 and float(stats[4]) == 0.0
    w = {"grpo": torch.repeat_interleave(1.0 / (n * torch.tensor(lengths).double()), torch.tensor(lengths)), "bnpo": torch.full((R,), 1.0 / R).double(),
         "dr_grpo": torch.full((R,), 1.0 / (n * MCL)).double()}[lt]
    want = -torch.repeat_interleave(adv.double(), torch.tensor(lengths)) * w
    assert bool(((dlogp[:R].double() - want).abs() <= 6 * GR.U * want.abs()).all())      # the weight's four roundings and the product
    fails, _ = GR.check_loss(dlogp[:R], stats[:8], logp, None, None, adv, so, 0.0, 0.0, 0.0, lt, MCL, 1.0)
    assert fails == [], fails
