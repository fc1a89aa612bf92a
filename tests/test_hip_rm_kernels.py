"""vlr_rm_head_fwd / vlr_rm_head_bwd (csrc/rm.hip) against fp64 host arithmetic: rewards within the fp32 accumulation bound, bit-equal
from call to call and between n = 1 and the same row inside n = 16; d hidden bit-equal to bf16(g * w) on the reward rows and untouched
elsewhere; d w / d b within one bf16 rounding of the fp64 sums, overwriting and accumulating.  Needs a real MI355X:  pytest -m gpu"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_hip_e2e import gpu  # noqa: E402,F401

HS = (8, 136, 2056, 4096)          # one 16-byte chunk; not a multiple of the 64-lane wave; past one sweep of the 256 threads (2048); the 7B width
NS = (1, 3, 16)
M = 24                             # rows of the hidden buffer
SENTINEL = -7.5


def _case(H, n, seed):
    """hidden [M][ldh > H] bf16, unsorted rows that include row 0 and the last row, head weight and a non-zero bias, upstream gradient"""
    g = torch.Generator().manual_seed(seed)
    ldh = H + 24
    hidden = torch.randn(M, ldh, generator=g).bfloat16()
    w = ((torch.rand(H, generator=g) * 2 - 1) / H ** 0.5).bfloat16()
    b = torch.tensor([0.3125]).bfloat16()
    rows = torch.randperm(M - 2, generator=g)[: max(n - 2, 0)] + 1
    rows = torch.cat([torch.tensor([M - 1]), rows, torch.tensor([0])])[:n] if n > 1 else torch.tensor([M - 1])
    d = torch.randn(n, generator=g)
    return hidden, ldh, rows.to(torch.int32), w, b, d


def _fwd(hip, hidden, ldh, rows, w, b, H):
    out = torch.empty(rows.numel(), dtype=torch.float32, device="cuda")
    hip.call("vlr_rm_head_fwd", hidden, ldh, rows, w, b, out, rows.numel(), H)
    return out


def _acc_bound(H, absdot):
    """fp32 accumulation of H products: 2 H 2^-24 sum |x_i w_i| (the bound of the issue's forward check)"""
    return 2 * H * 2.0 ** -24 * absdot


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("n", NS)
def test_rm_head_fwd(gpu, H, n):
    from vlrlhf import _hip as hip
    hidden, ldh, rows, w, b, _ = _case(H, n, seed=H + n)
    dev = [t.cuda() for t in (hidden, rows, w, b)]
    got = _fwd(hip, dev[0], ldh, dev[1], dev[2], dev[3], H)
    again = _fwd(hip, dev[0], ldh, dev[1], dev[2], dev[3], H)
    torch.cuda.synchronize()
    assert torch.equal(got, again)                                     # fixed reduction order: the same bits from call to call
    x = hidden[rows.long(), :H].double()
    exp = x @ w.double() + b.double()
    bound = _acc_bound(H, (x.abs() @ w.double().abs())) + 2.0 ** -23 * exp.abs()
    err = (got.cpu().double() - exp).abs()
    print(f"[rm fwd] H={H} n={n} worst err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), (err, bound)
    if H > 8:                                                          # fp32 out, never rounded to bf16
        assert bool((got.cpu() != got.cpu().bfloat16().float()).any())


@pytest.mark.parametrize("H", HS)
def test_rm_head_fwd_row_bits_do_not_depend_on_n(gpu, H):
    from vlrlhf import _hip as hip
    hidden, ldh, rows, w, b, _ = _case(H, 16, seed=H)
    dev = [t.cuda() for t in (hidden, w, b)]
    all16 = _fwd(hip, dev[0], ldh, rows.cuda(), dev[1], dev[2], H)
    for i in (0, 7, 15):
        one = _fwd(hip, dev[0], ldh, rows[i:i + 1].cuda(), dev[1], dev[2], H)
        assert torch.equal(one, all16[i:i + 1]), (H, i)


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("n", NS)
def test_rm_head_bwd(gpu, H, n):
    from vlrlhf import _hip as hip
    hidden, ldh, rows, w, b, d = _case(H, n, seed=3 * H + n)
    ldd = H + 8
    hd, rd, wd, dd = hidden.cuda(), rows.cuda(), w.cuda(), d.cuda()
    x = hidden[rows.long(), :H].double()
    exp_dw, exp_db = d.double() @ x, d.double().sum()
    absdw, absdb = d.double().abs() @ x.abs(), d.double().abs().sum()
    old_w = torch.randn(H, generator=torch.Generator().manual_seed(1)).bfloat16()
    old_b = torch.tensor([0.75]).bfloat16()
    for acc in (0, 1):
        dh = torch.full((M, ldd), SENTINEL, dtype=torch.bfloat16, device="cuda")
        dw, db = old_w.clone().cuda(), torch.cat([old_b, torch.full((7,), SENTINEL).bfloat16()]).cuda()
        hip.call("vlr_rm_head_bwd", hd, ldh, rd, wd, dd, dh, ldd, dw, db, acc, n, H)
        torch.cuda.synchronize()
        dh = dh.cpu()
        assert torch.equal(dh[rows.long(), :H], (d.float()[:, None] * w.float()[None, :]).bfloat16())      # bf16(g * w), bit for bit
        rest = torch.ones(M, ldd, dtype=torch.bool)
        rest[rows.long(), :H] = False
        assert bool((dh[rest].float() == SENTINEL).all())                # no other row, and nothing past column H of a reward row
        tw = exp_dw + (old_w.double() if acc else 0)
        tb = exp_db + (old_b.double() if acc else 0)
        # one bf16 rounding (unit roundoff 2^-8) of the fp64 value + the fp32 accumulation of n (+ 1) terms
        bw = 2.0 ** -8 * tw.abs() + _acc_bound(n + 1, absdw + old_w.double().abs() * acc)
        bb = 2.0 ** -8 * tb.abs() + _acc_bound(n + 1, absdb + old_b.double().abs() * acc)
        ew, eb = (dw.cpu().double() - tw).abs(), (db.cpu()[:1].double() - tb).abs()
        print(f"[rm bwd] H={H} n={n} acc={acc} worst dw err/bound {float((ew / bw.clamp_min(1e-30)).max()):.3f} db {float(eb / bb):.3f}")
        assert bool((ew <= bw).all()) and bool((eb <= bb).all()), (acc, float(ew.max()), float(eb))
        assert bool((db.cpu()[1:].float() == SENTINEL).all())            # the bias gradient is ONE element
    # a zero upstream gradient gives zero rows (and zero head gradients)
    dh = torch.full((M, ldd), SENTINEL, dtype=torch.bfloat16, device="cuda")
    dw, db = old_w.clone().cuda(), old_b.clone().cuda()
    hip.call("vlr_rm_head_bwd", hd, ldh, rd, wd, torch.zeros(n, device="cuda"), dh, ldd, dw, db, 0, n, H)
    torch.cuda.synchronize()
    assert float(dh[rd.long(), :H].float().abs().sum()) == 0.0 and float(dw.float().abs().sum()) == 0.0 and float(db.float().abs().sum()) == 0.0
