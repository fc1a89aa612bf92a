"""vlr_kto_loss (csrc/kto.hip) against the fp64 host arithmetic of tests/kto_ref.py at the edges of its loops.  The one comparison is
kto_ref.check, whose bounds are formulas of the fp32 unit roundoff, the depth of the sums the header documents (lane-strided partials,
six xor butterflies, sixteen waves in order), the magnitude of the terms and expf's 2 ulp; tests/test_kto_checker_host.py shows that it
flags planted faults.  Needs a real MI355X:  pytest -m gpu"""
import os

import pytest
import torch

from tests import kto_ref as KR

pytestmark = pytest.mark.gpu

from tests.test_hip_e2e import gpu  # noqa: E402,F401

SENTINEL = -7.5
BETA, W_D, W_U = 0.1, 1.25, 0.75
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kto.txt")
_worst = {"ratio": 0.0, "case": ""}


def _run(hip, pi, ref, label, pi_kl, ref_kl, beta=BETA, w_d=W_D, w_u=W_U, up=1.0):
    n, m = pi.numel(), pi_kl.numel()
    out = [torch.full((n + 8,), SENTINEL, device="cuda") for _ in range(3)]
    stats = torch.full((16,), SENTINEL, device="cuda")
    hip.call("vlr_kto_loss", pi.cuda(), ref.cuda(), label.cuda(), n, pi_kl.cuda(), ref_kl.cuda(), m, beta, w_d, w_u, up, *out, stats)
    torch.cuda.synchronize()
    return [t.cpu() for t in out] + [stats.cpu()]


def _checked(hip, inp, up, tag, **kw):
    n = inp[0].numel()
    got = _run(hip, *inp, up=up, **kw)
    again = _run(hip, *inp, up=up, **kw)
    assert all(torch.equal(a, b) for a, b in zip(got, again))                 # fixed reduction order: the same bits from call to call
    assert all(bool((t[n:] == SENTINEL).all()) for t in got[:3]) and bool((got[3][8:] == SENTINEL).all())
    fails, worst = KR.check(got[0][:n], got[1][:n], got[2][:n], got[3][:8], *inp, kw.get("beta", BETA), kw.get("w_d", W_D), kw.get("w_u", W_U), up)
    print(f"[kto loss] {tag} worst err/bound {worst:.3f}")
    assert fails == [], fails
    if worst > _worst["ratio"]:
        _worst.update(ratio=worst, case=tag)
    return got


@pytest.fixture(scope="module", autouse=True)
def _record_worst():
    """appends the worst error-to-bound ratio of this module's run to profiles/kto.txt"""
    yield
    if _worst["ratio"] > 0:
        with open(PROFILE, "a") as f:
            f.write(f"tests/test_hip_kto_kernels.py: worst |error| / bound of vlr_kto_loss against the fp64 replay {_worst['ratio']:.3f} "
                    f"({_worst['case']}; 1 box, 1 run)\n")


# n: one row; two; one below, at and above a wave; one below, at and above the workgroup's 1024 threads; a third sweep of the lanes
@pytest.mark.parametrize("labels", ["ones", "zeros", "mixed"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_kto_loss_rows(gpu, n, labels):
    from vlrlhf import _hip as hip
    inp = KR.make_inputs(n, 65, labels, BETA, 1.5, seed=n)
    cnt = KR.branch_counts(*inp, BETA)
    assert sum(cnt.values()) == n
    if n >= 63:      # every |beta (r - kl)|: flat (0.25 .. 1), around 1, at 30 (mid) and at 200 (saturated), under the labels present
        want = [b for b in KR.BRANCHES if labels == "mixed" or b.startswith("desirable" if labels == "ones" else "undesirable")]
        assert all(cnt[b] >= 7 for b in want), cnt
    got = _checked(hip, inp, 0.25, f"n={n} m=65 labels={labels} branches {cnt}")
    lab = inp[2].bool()
    assert float(got[3][6]) == float(lab.sum()) and float(got[3][7]) == float((~lab).sum())
    if labels != "mixed":      # a class that does not occur: its sums are exactly 0, and the mean is still over n
        empty = (3, 5) if labels == "ones" else (2, 4)
        assert all(float(got[3][i]) == 0.0 for i in empty)


# m: one KL row; a wave; one above it; one above the workgroup
@pytest.mark.parametrize("kl_mean", [1.5, -2.0])
@pytest.mark.parametrize("m", [1, 64, 65, 1025])
def test_kto_loss_kl_rows(gpu, m, kl_mean):
    from vlrlhf import _hip as hip
    inp = KR.make_inputs(65, m, "mixed", BETA, kl_mean, seed=1000 + m)
    got = _checked(hip, inp, 1.0, f"n=65 m={m} kl_mean={kl_mean}")
    if kl_mean < 0:
        # a negative mean log-ratio on the KL rows: kl is exactly 0 and every output is that of KL rows whose log-ratio IS 0
        assert float(got[3][1]) == 0.0
        zero = _run(hip, inp[0], inp[1], inp[2], inp[4].clone(), inp[4])
        assert all(torch.equal(a, b) for a, b in zip(got, zero))
    else:
        assert float(got[3][1]) > 0.0


def test_kto_loss_saturated_is_exact_and_finite(gpu):
    """|beta (r - kl)| = 200 on both sides and both labels: the loss is exactly w or 0, the gradient exactly 0, everything finite"""
    from vlrlhf import _hip as hip
    ref = torch.full((4,), -50.0)
    pi = ref + torch.tensor([2000.0, -2000.0, 2000.0, -2000.0])
    label = torch.tensor([1, 1, 0, 0], dtype=torch.uint8)
    losses, rewards, dpi, stats = _run(hip, pi, ref, label, torch.zeros(3), torch.zeros(3), up=0.5)
    assert losses[:4].tolist() == [0.0, W_D, W_U, 0.0] and dpi[:4].tolist() == [0.0] * 4
    assert rewards[:4].tolist() == [200.0, -200.0, 200.0, -200.0]
    assert bool(torch.isfinite(stats[:8]).all()) and float(stats[0]) == (W_D + W_U) / 4 and float(stats[1]) == 0.0


@pytest.mark.parametrize("n", [64, 1024, 65])
def test_kto_loss_zero_log_ratio_is_exact(gpu, n):
    """pi == ref and pi_kl == ref_kl bit for bit: every loss is exactly w / 2, every reward 0, every gradient -+ w beta / (4 n) upstream"""
    from vlrlhf import _hip as hip
    g = torch.Generator().manual_seed(n)
    pi, pk = -300 * torch.rand(n, generator=g), -300 * torch.rand(7, generator=g)
    label = (torch.arange(n) % 3 != 0).to(torch.uint8)
    beta, up = 0.25, 0.5                                       # powers of two: with n = 64 or 1024 the weight is exact in fp32
    losses, rewards, dpi, stats = _run(hip, pi, pi.clone(), label, pk, pk.clone(), beta=beta, up=up)
    lab = label.bool()
    w = torch.where(lab, torch.tensor(W_D), torch.tensor(W_U))
    assert torch.equal(losses[:n], 0.5 * w) and bool((rewards[:n] == 0).all()) and float(stats[1]) == 0.0
    sign = torch.where(lab, -1.0, 1.0).double()
    want = sign * w.double() * beta / (4.0 * n) * up
    if n in (64, 1024):
        assert torch.equal(dpi[:n].double(), want)
    else:      # ((w beta) / n) upstream: the division rounds once, the other factors are exact here
        assert bool(((dpi[:n].double() - want).abs() <= KR.U * want.abs()).all())
    assert float(stats[2]) == 0.0 and float(stats[3]) == 0.0 and float(stats[6]) == float(lab.sum())


def test_kto_loss_refusals_launch_nothing(gpu):
    """every argument the header refuses returns the argument error; the outputs keep their sentinel"""
    from vlrlhf import _hip as hip
    n = m = 4
    t = lambda: torch.full((n,), SENTINEL, device="cuda")      # noqa: E731
    pi, ref, pk, rk, lo, rw, dp = (t() for _ in range(7))
    lab = torch.ones(n, dtype=torch.uint8, device="cuda")
    stats = torch.full((8,), SENTINEL, device="cuda")
    good = [pi, ref, lab, n, pk, rk, m, 0.1, 1.0, 1.0, 1.0, lo, rw, dp, stats]
    hip.call("vlr_kto_loss", *good)
    torch.cuda.synchronize()
    assert float(stats[6]) == 4.0
    for t_ in (lo, rw, dp, stats):
        t_.fill_(SENTINEL)
    bad = []
    for i in (0, 1, 2, 4, 5, 11, 12, 13, 14):
        bad.append((i, None, "null operand"))
    bad += [(3, 0, "bad shape"), (3, -1, "bad shape"), (3, (1 << 20) + 1, "bad shape"), (6, 0, "bad shape"), (6, (1 << 20) + 1, "bad shape")]
    for i in (7, 8, 9, 10):
        bad += [(i, float("nan"), "not finite"), (i, float("inf"), "not finite")]
    for i, v, msg in bad:
        args = list(good)
        args[i] = v
        with pytest.raises(ValueError, match=msg):
            hip.call("vlr_kto_loss", *args)
    torch.cuda.synchronize()
    assert all(bool((t_ == SENTINEL).all()) for t_ in (lo, rw, dp, stats))
