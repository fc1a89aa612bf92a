"""vlr_lmhead_logps_entropy_fwd / _bwd (fuse = 8 | 9 of csrc/gemm256p.hip, lmhead_ent_fold_kernel, the row kernels of csrc/dpo_ops.hip)
and vlr_grpo_loss_ent (csrc/grpo.hip) through the C ABI, against the fp64 reference and the derived bounds of tests/entropy_ref.py
(tests/test_entropy_checker_host.py shows that those checks flag planted faults) and, bit for bit, against the entry points they sit
beside.  Each shape runs once; the tests below read that one run.  Needs a real MI355X:  pytest -m gpu"""
import math

import pytest
import torch

from tests import entropy_ref as ER
from tests import grpo_ref as GR

pytestmark = pytest.mark.gpu

from tests.test_hip_e2e import gpu  # noqa: E402,F401
from tests.test_hip_grpo_kernels import ADV_CYCLE, BETA, EPS_HIGH, EPS_LOW, LOSS_CASES, MCL  # noqa: E402

NAN = float("nan")
_runs = {}


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _forward(hip, c, R, V, H, fused_route, entropy=True):
    """-> (tok, lse, H) [R + 4] each, prefilled with NaN: the 4 guard rows behind R must stay"""
    tok, lse, ent = _nan(R + 4), _nan(R + 4), _nan(R + 4)
    nbytes = int(hip.lib().vlr_lmhead_entropy_workspace_bytes(R, V)) if entropy else int(hip.lib().vlr_lmhead_workspace_bytes(R, V))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda") if fused_route else None
    logits = None if fused_route else torch.empty(R, V, dtype=torch.float32, device="cuda")
    if entropy:
        hip.call("vlr_lmhead_logps_entropy_fwd", c["hg"], c["w"], c["tgt"], tok, lse, ent, ws, logits, R, V, H)
    else:
        hip.call("vlr_lmhead_logps_fwd", c["hg"], c["w"], c["tgt"], tok, lse, ws, logits, R, V, H)
    torch.cuda.synchronize()
    return tok, lse, ent


def _backward(hip, c, R, V, H, fused_route, lse, ent, dlogp, dent):
    """-> d logits [R + 2][V] bf16 prefilled with NaN; dent None: vlr_lmhead_logps_bwd with nseq = R, seq_off = 0..R, average = 0"""
    dl = _nan(R + 2, V, dtype=torch.bfloat16)
    ws = torch.empty(int(hip.lib().vlr_lmhead_entropy_workspace_bytes(R, V)), dtype=torch.uint8, device="cuda") if fused_route else None
    logits = None if fused_route else torch.empty(R, V, dtype=torch.float32, device="cuda")
    if dent is None:
        so = torch.arange(R + 1, dtype=torch.int32, device="cuda")
        hip.call("vlr_lmhead_logps_bwd", c["hg"], c["w"], c["tgt"], lse, so, R, dlogp, 0, dl, ws, logits, R, V, H)
    else:
        hip.call("vlr_lmhead_logps_entropy_bwd", c["hg"], c["w"], c["tgt"], lse, ent, dlogp, dent, dl, ws, logits, R, V, H)
    torch.cuda.synchronize()
    return dl


def _run(shape):
    if shape in _runs:
        return _runs[shape]
    from vlrlhf import _hip as hip
    R, V, H, fused = shape
    assert bool(hip.helper("vlr_lmhead_is_fused", R, V, H)) == fused
    c = ER.make_case(R, V, H, seed=R + V + H, device="cuda")
    g = torch.Generator().manual_seed(11)
    c["dlogp"], c["dent"] = torch.randn(R, generator=g).cuda(), torch.randn(R, generator=g).cuda()
    c["ref"] = ER.forward_reference(c["hg"], c["w"], c["tgt"])
    zero = torch.zeros(R, device="cuda")
    c["fwd"] = _forward(hip, c, R, V, H, fused)
    c["fwd_again"] = _forward(hip, c, R, V, H, fused)
    c["fwd_old"] = _forward(hip, c, R, V, H, fused, entropy=False)
    lse, ent = c["fwd"][1][:R].contiguous(), c["fwd"][2][:R].contiguous()
    c["bwd_old"] = _backward(hip, c, R, V, H, fused, lse, None, c["dlogp"], None)
    c["bwd_dent0"] = _backward(hip, c, R, V, H, fused, lse, ent, c["dlogp"], zero)
    c["bwd_dlogp0"] = _backward(hip, c, R, V, H, fused, lse, ent, zero, c["dent"])
    c["bwd_both"] = _backward(hip, c, R, V, H, fused, lse, ent, c["dlogp"], c["dent"])
    c["bwd_again"] = _backward(hip, c, R, V, H, fused, lse, ent, c["dlogp"], c["dent"])
    if fused:                                                  # (e) the same problem through the logits buffer and the row kernels
        c["fwd_rows"] = _forward(hip, c, R, V, H, False)
        c["bwd_rows"] = _backward(hip, c, R, V, H, False, lse, ent, c["dlogp"], c["dent"])
    _runs[shape] = c
    return c


@pytest.mark.parametrize("shape", ER.SHAPES)
def test_logps_and_lse_are_the_bits_of_the_entry_point_without_entropy(gpu, shape):
    """(a), (f), (g) of the forward"""
    R = shape[0]
    c = _run(shape)
    for new, old, what in zip(c["fwd"][:2], c["fwd_old"][:2], ("tok_logp", "lse")):
        assert bool(torch.isfinite(new[:R]).all()), what
        assert torch.equal(_bits(new[:R]), _bits(old[:R])), what
    for t in c["fwd"]:
        assert bool(torch.isnan(t[R:]).all()) and bool(torch.isfinite(t[:R]).all())       # fully written, nothing behind R
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(c["fwd"], c["fwd_again"]))


@pytest.mark.parametrize("shape", ER.SHAPES)
def test_entropy_within_the_derived_bound(gpu, shape):
    """(b): within the bound of fp64 and of [0, log V]; the planted rows by their closed forms"""
    R, V, H, _ = shape
    c = _run(shape)
    ent = c["fwd"][2][:R]
    fails, worst = ER.check_entropy(ent, c["ref"], V)
    print(f"[entropy] {shape} worst err/bound {worst:.3f}; largest bound {float(c['ref']['b_H'].max()):.3g}, largest logit error bound "
          f"{float(c['ref']['ez'].max()):.3g}")
    assert fails == [], fails
    for r, kind in enumerate(c["kinds"]):
        if kind == "zero":
            assert abs(float(ent[r]) - math.log(V)) <= 4 * ER.U * math.log(V)
        elif kind.startswith("dom@"):
            assert float(ent[r]) == 0.0 and float(c["fwd"][0][r]) == 0.0               # every other column underflows: H = 0, log p = 0
        elif kind == "tie":
            assert abs(float(ent[r]) - float(c["ref"]["H"][r])) <= float(c["ref"]["b_H"][r])


@pytest.mark.parametrize("shape", ER.SHAPES)
def test_backward_with_zero_dent_is_the_bits_of_the_entry_point_without_entropy(gpu, shape):
    """(c), (f), (g) of the backward"""
    R, V = shape[0], shape[1]
    c = _run(shape)
    assert torch.equal(_bits(c["bwd_dent0"][:R]), _bits(c["bwd_old"][:R]))
    for name in ("bwd_dent0", "bwd_dlogp0", "bwd_both"):
        assert bool(torch.isfinite(c[name][:R].float()).all()), name                    # every element written
        assert bool(torch.isnan(c[name][R:].float()).all()), name                       # the guard rows behind R untouched
    assert torch.equal(_bits(c["bwd_both"]), _bits(c["bwd_again"]))


@pytest.mark.parametrize("shape", ER.SHAPES)
@pytest.mark.parametrize("which", ["bwd_dlogp0", "bwd_both"])
def test_backward_within_the_derived_bound(gpu, shape, which):
    """(d)"""
    R = shape[0]
    c = _run(shape)
    dlogp = torch.zeros_like(c["dlogp"]) if which == "bwd_dlogp0" else c["dlogp"]
    fails, worst = ER.check_dlogits(c[which][:R], c["hg"], c["w"], c["tgt"], c["ref"], dlogp, c["dent"])
    print(f"[entropy bwd] {shape} {which} worst err/bound {worst:.3f}")
    assert fails == [], fails


@pytest.mark.parametrize("shape", [s for s in ER.SHAPES if s[3]])
def test_fused_shape_through_the_unfused_route(gpu, shape):
    """(e): both routes are within their bound of the reference, so of each other within the sum"""
    R, V = shape[0], shape[1]
    c = _run(shape)
    ent_f, ent_r = c["fwd"][2][:R].double(), c["fwd_rows"][2][:R].double()
    assert bool(((ent_f - ent_r).abs() <= 2 * c["ref"]["b_H"]).all())
    assert bool(((c["fwd"][1][:R].double() - c["fwd_rows"][1][:R].double()).abs() <= 2 * c["ref"]["b_lse"]).all())
    fails, _ = ER.check_entropy(c["fwd_rows"][2][:R], c["ref"], V, "entropy (row kernel)")
    assert fails == [], fails
    fails, worst = ER.check_dlogits(c["bwd_rows"][:R], c["hg"], c["w"], c["tgt"], c["ref"], c["dlogp"], c["dent"], "dlogits (row kernel)")
    print(f"[entropy bwd] {shape} row kernels worst err/bound {worst:.3f}")
    assert fails == [], fails
    assert bool(torch.isnan(c["bwd_rows"][R:].float()).all()) and bool(torch.isnan(c["fwd_rows"][2][R:]).all())


def test_row_kernel_leaves_the_guard_columns(gpu):
    """vlr_dlogits_ent_rows with a destination pitch wider than V: the 8 columns behind V of every row stay as they were"""
    from vlrlhf import _hip as hip
    R, V, H, _ = ER.SHAPES[3]
    c = _run(ER.SHAPES[3])
    logits = (c["hg"].float() @ c["w"].float().t()).contiguous()
    dl = _nan(R + 1, V + 8, dtype=torch.bfloat16)
    hip.call("vlr_dlogits_ent_rows", logits, c["tgt"], c["fwd"][1], c["fwd"][2], c["dlogp"], c["dent"], R, V, V, dl, V + 8)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dl[:R, :V].float()).all()) and bool(torch.isnan(dl[:R, V:].float()).all()) and bool(torch.isnan(dl[R:].float()).all())
    fails, _ = ER.check_dlogits(dl[:R], c["hg"], c["w"], c["tgt"], c["ref"], c["dlogp"], c["dent"])
    assert fails == [], fails


# ------------------------------------------------------------------------------------------------------------ vlr_grpo_loss_ent
SENTINEL = -7.5


def _run_ent(hip, logp, old, ref, adv, so, beta, lt, up, ent, keep, coef, want_dent=True):
    R, n = logp.numel(), len(so) - 1
    dev = lambda t: None if t is None else t.cuda()            # noqa: E731
    dlogp = torch.full((R + 8,), SENTINEL, device="cuda")
    dent = torch.full((R + 8,), SENTINEL, device="cuda") if want_dent else None
    stats = torch.full((16,), SENTINEL, device="cuda")
    hip.call("vlr_grpo_loss_ent", logp.cuda(), dev(old), dev(ref), adv.cuda(), torch.tensor(so, dtype=torch.int32).cuda(), R, n, EPS_LOW, EPS_HIGH,
             beta, GR.LOSS_TYPES[lt], MCL, up, dev(ent), None if keep is None else keep.to(torch.uint8).cuda(), coef, dlogp, dent, stats)
    torch.cuda.synchronize()
    return dlogp.cpu(), None if dent is None else dent.cpu(), stats.cpu()


ENT_CASES = ["R1", "n_eq_R_past_the_waves", "one_token_among_long", "branches"]      # n = 1; one-token sequences, more than the waves; mixed


@pytest.mark.parametrize("mask", ["ones", "zeros", "random"])
@pytest.mark.parametrize("lt", sorted(GR.LOSS_TYPES))
@pytest.mark.parametrize("case", ENT_CASES)
def test_grpo_loss_ent(gpu, case, lt, mask):
    from vlrlhf import _hip as hip
    lengths = LOSS_CASES[case]
    logp, old, ref, adv, so = GR.branch_inputs(lengths, ADV_CYCLE, EPS_LOW, EPS_HIGH, seed=sum(lengths) + len(lengths))
    R = sum(lengths)
    g = torch.Generator().manual_seed(R)
    ent = torch.rand(R, generator=g) * 4
    keep = dict(ones=torch.ones(R, dtype=torch.bool), zeros=torch.zeros(R, dtype=torch.bool), random=torch.rand(R, generator=g) < 0.5)[mask]
    coef, up = 0.02, 0.5
    for o, rf, beta in ((old, ref, BETA), (None, None, 0.0)):
        got = _run_ent(hip, logp, o, rf, adv, so, beta, lt, up, ent, keep, coef)
        again = _run_ent(hip, logp, o, rf, adv, so, beta, lt, up, ent, keep, coef)
        assert all(torch.equal(a, b) for a, b in zip(got, again))
        dlogp, dent, stats = got
        assert bool((dlogp[R:] == SENTINEL).all()) and bool((dent[R:] == SENTINEL).all()) and bool((stats[10:] == SENTINEL).all())
        fails, worst = ER.check_grpo_ent(dlogp[:R], dent[:R], stats[:10], logp, o, rf, adv, so, EPS_LOW, EPS_HIGH, beta, lt, MCL, up, ent, keep, coef)
        print(f"[grpo ent] {case} {lt} {mask} beta={beta} worst err/bound {worst:.3f}")
        assert fails == [], fails
        if mask == "zeros":                                    # the loss is the bonus alone, no token carries a policy gradient
            assert bool((dlogp[:R] == 0).all()) and float(stats[9]) == 0.0 and float(stats[0]) < 0
        if mask == "ones":
            assert float(stats[9]) == 1.0


@pytest.mark.parametrize("beta", [0.0, BETA])
@pytest.mark.parametrize("lt", sorted(GR.LOSS_TYPES))
@pytest.mark.parametrize("case", ENT_CASES)
def test_grpo_loss_ent_without_mask_and_bonus_is_vlr_grpo_loss(gpu, case, lt, beta):
    from vlrlhf import _hip as hip
    lengths = LOSS_CASES[case]
    logp, old, ref, adv, so = GR.branch_inputs(lengths, ADV_CYCLE, EPS_LOW, EPS_HIGH, seed=sum(lengths) + len(lengths))
    R, n = sum(lengths), len(lengths)
    for o in (old, None):
        dlogp = torch.full((R,), SENTINEL, device="cuda")
        stats = torch.full((8,), SENTINEL, device="cuda")
        hip.call("vlr_grpo_loss", logp.cuda(), None if o is None else o.cuda(), ref.cuda() if beta else None, adv.cuda(),
                 torch.tensor(so, dtype=torch.int32).cuda(), R, n, EPS_LOW, EPS_HIGH, beta, GR.LOSS_TYPES[lt], MCL, 0.25, dlogp, stats)
        torch.cuda.synchronize()
        ent = torch.rand(R) * 4
        for e, want_dent in ((None, False), (ent, True)):      # entropy NULL (no stat wanted) and given: the same loss bits
            got = _run_ent(hip, logp, o, ref if beta else None, adv, so, beta, lt, 0.25, e, None, 0.0, want_dent)
            assert torch.equal(_bits(got[0][:R]), _bits(dlogp.cpu())) and torch.equal(_bits(got[2][:8]), _bits(stats.cpu()))
            assert float(got[2][9]) == 1.0
            if e is None:
                assert float(got[2][8]) == 0.0
            else:
                assert bool((got[1][:R] == 0).all()) and abs(float(got[2][8]) - float(ent.double().mean())) <= 64 * ER.U * 4
