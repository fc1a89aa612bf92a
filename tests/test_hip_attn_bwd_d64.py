"""vlr_attn_bwd at head_dim 64 (the CLIP ViT's width; attn_bwd_dq_kernel<64> / attn_bwd_dkv_kernel<64> / attn_delta_kernel<64> of
csrc/attention.hip) against the fp64 reference and the per-tile checker of tests/attn_ref.py.

Cases: S in {1, 17, 63, 64, 65, 129, 577} (one row, less than a 32-row wave, the 64-row LDS tile and its neighbours, more than one
128-row workgroup, CLIP-L's 577 tokens) x {full attention, full attention with padded keys, causal} at B = 2, heads = 2; CLIP-L's 16
heads at S = 577; one score-range case (a sink key ~40 above the rest, as the D = 128 suite has).

Bound: attn_ref.TOL of the case's group ("lengths", "scores"), the per-tile tolerances tests/test_hip_attention_edges.py applies to its
D = 128 backward cases.  They are ~2x the worst error of attn_ref.emulate_kernel_rounding (bf16 operands, P and dS rounded to bf16, bf16
outputs) against the fp64 reference; none of those roundings depends on D, the fp32 accumulation over D is shorter here, and the test
below checks on the CPU that the same model at D = 64 passes the same numbers.

Every output starts as NaN, so an unwritten row shows; the gradients are column blocks of one buffer whose row stride is wider than
3 * heads * 64, with poisoned columns on both sides of each block, so a store past a block shows.  GPU tests need a real MI355X:
pytest -m gpu"""
import math

import pytest
import torch

from tests import attn_ref as A

DEV = "cuda"
D = 64
POISON = 768.0          # exact in bf16; a gradient of the O(1) inputs never equals it
BORDER = 8              # columns (16 bytes: the blocks stay 16-byte aligned)


def _cases():
    out = []
    for S in (1, 17, 63, 64, 65, 129, 577):
        out.append(A._case("lengths", 2, S, D=D, causal=False, kind="none"))
        if S > 8:
            out.append(A._case("lengths", 2, S, D=D, causal=False, kind="right"))
        out.append(A._case("lengths", 2, S, D=D, causal=True, kind="right" if S > 8 else "none"))
    out.append(A._case("lengths", 1, 577, nh=16, D=D, causal=False, kind="none"))
    out.append(A._case("scores", 1, 129, D=D, causal=False, scores="sink", kind="right"))
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return _hip


def run_bwd64(hip, c, q, k, v, do, km):
    """forward (for O and lse) and backward of case c -> Attn; checks the padded rows of lse / delta and the poisoned border columns"""
    B, S, nh = c.B, c.S, c.nh
    H = nh * D
    Sp = (S + 63) // 64 * 64
    scale = 1.0 / math.sqrt(D)
    qkv = torch.cat([x.reshape(B * S, H) for x in (q, k, v)], 1).to(DEV).contiguous()
    dod = do.reshape(B * S, H).to(DEV).contiguous()
    kmd = None if km is None else km.to(DEV)
    o = torch.full((B * S, H), float("nan"), dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B, nh, Sp), float("nan"), dtype=torch.float32, device=DEV)
    hip.call("vlr_attn_fwd", qkv, qkv[:, H:], qkv[:, 2 * H:], 3 * H, o, H, lse, kmd, B, S, nh, D, int(c.causal), scale)
    ldd = 3 * H + 4 * BORDER
    cols = [BORDER + j * (H + BORDER) for j in range(3)]                 # first column of dq, dk, dv
    d = torch.full((B * S, ldd), float("nan"), dtype=torch.bfloat16, device=DEV)
    border = torch.ones(ldd, dtype=torch.bool)
    for c0 in cols:
        border[c0:c0 + H] = False
    d[:, border.to(DEV)] = POISON
    delta = torch.full((B, nh, Sp), float("nan"), dtype=torch.float32, device=DEV)
    hip.call("vlr_attn_bwd", qkv, qkv[:, H:], qkv[:, 2 * H:], 3 * H, o, dod, H, lse, delta, kmd, d[:, cols[0]:], d[:, cols[1]:], d[:, cols[2]:],
             ldd, B, S, nh, D, int(c.causal), scale)
    torch.cuda.synchronize()
    assert bool((lse[:, :, S:] == math.inf).all())
    assert bool(torch.isfinite(delta).all()) and float(delta[:, :, S:].abs().max() if Sp > S else 0.0) == 0.0
    assert bool((d[:, border.to(DEV)] == POISON).all()), "a store outside the dq / dk / dv column blocks"
    dq, dk, dv = (d[:, c0:c0 + H].reshape(B, S, nh, D) for c0 in cols)
    return A.Attn(o.reshape(B, S, nh, D), lse[:, :, :S].transpose(1, 2), dq, dk, dv, None, None, None)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_attn_bwd_d64_parity(hip, c):
    q, k, v, do, km = A.make_inputs(c, seed=1)
    res = run_bwd64(hip, c, q, k, v, do, km)
    kmd = None if km is None else km.to(DEV)
    ref = A.ref_attention(q.to(DEV), k.to(DEV), v.to(DEV), kmd, c.causal, do=do.to(DEV), o_bwd=res.o)
    worst = A.check_attention(res, ref, A.TOL[c.group], c.name)
    print(c.name, " ".join(f"{n}={e:.2e}" for n, e in worst.items()))


@pytest.mark.gpu
def test_attn_bwd_d64_is_deterministic_and_refuses_gqa(hip):
    """fixed accumulation order, no atomics: two calls give the same bits; grouped-query attention at 64 stays refused"""
    c = A._case("lengths", 2, 129, D=D, causal=False, kind="right")
    q, k, v, do, km = A.make_inputs(c, seed=2)
    a, b = run_bwd64(hip, c, q, k, v, do, km), run_bwd64(hip, c, q, k, v, do, km)
    for x, y in ((a.dq, b.dq), (a.dk, b.dk), (a.dv, b.dv)):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))
    t = torch.zeros(64, 4 * D, dtype=torch.bfloat16, device=DEV)
    f = torch.zeros(1, 2, 64, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="head_dim 64"):
        hip.call("vlr_attn_bwd_gqa", t, t[:, 2 * D:], t[:, 3 * D:], 4 * D, t, t, 2 * D, f, f, None, t, t[:, 2 * D:], t[:, 3 * D:], 4 * D,
                 1, 64, 2, 1, D, 0, 0.125)


# ---------------------------------------------------------------------------------------------------- the checker at D = 64, on the CPU
def _autograd64(q, k, v, do, km, causal):
    """torch autograd in float64 of softmax(q k^T / sqrt(D) + mask) v, [B, S, nh, D] layout"""
    B, S, nh, _ = q.shape
    q, k, v = (x.double().clone().requires_grad_(True) for x in (q, k, v))
    s = torch.einsum("bihd,bjhd->bhij", q, k) / math.sqrt(D)
    vis = torch.stack([A.visibility(S, None if km is None else km[b], causal, "cpu") for b in range(B)])[:, None]
    p = torch.softmax(s.masked_fill(~vis, -math.inf), -1)
    p = torch.where(vis.any(-1, keepdim=True), p, torch.zeros_like(p))        # a row that sees no key: O = 0
    o = torch.einsum("bhij,bjhd->bihd", p, v)
    (o * do.double()).sum().backward()
    return o.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("S,causal,kind", [(17, False, "right"), (65, True, "right"), (129, False, "none")])
def test_reference_at_d64_matches_autograd(S, causal, kind):
    c = A._case("lengths", 2, S, D=D, causal=causal, kind=kind)
    q, k, v, do, km = A.make_inputs(c, seed=3)
    ref = A.ref_attention(q, k, v, km, causal, do=do)
    o, dq, dk, dv = _autograd64(q, k, v, do, km, causal)
    for name, x, y in (("o", ref.o, o), ("dq", ref.dq, dq), ("dk", ref.dk, dk), ("dv", ref.dv, dv)):
        assert float((x - y).abs().max()) < 1e-11, name


def test_rounding_model_at_d64_passes_the_bound_and_a_dropped_key_tile_fails():
    """the kernels' rounding model at D = 64 is inside the D = 128 suite's tolerances (so the bound is not too tight for a correct
    kernel at this width), and the checker flags a planted fault: the last, partial key tile dropped"""
    for c in (A._case("lengths", 2, 129, D=D, causal=False, kind="right"), A._case("lengths", 2, 65, D=D, causal=True, kind="right"),
              A._case("scores", 1, 129, D=D, causal=False, scores="sink", kind="right")):
        q, k, v, do, km = A.make_inputs(c, seed=1)
        emu = A.emulate_kernel_rounding(q, k, v, km, c.causal, do=do)
        ref = A.ref_attention(q, k, v, km, c.causal, do=do, o_bwd=emu.o)
        worst = A.check_attention(emu, ref, A.TOL[c.group], c.name)
        print(c.name, " ".join(f"{n}={e:.2e}" for n, e in worst.items()))
    c = A._case("lengths", 2, 129, D=D, causal=False, kind="none")
    q, k, v, do, km = A.make_inputs(c, seed=1)
    bad = A.emulate_kernel_rounding(q, k, v, km, c.causal, do=do, bug="tail_tile_ignored")
    ref = A.ref_attention(q, k, v, km, c.causal, do=do, o_bwd=bad.o)
    for name, x, y, z in (("dq", bad.dq, ref.dq, ref.zero_dq), ("dk", bad.dk, ref.dk, ref.zero_kv), ("dv", bad.dv, ref.dv, ref.zero_kv)):
        with pytest.raises(AssertionError):
            A.check_tiles(x, y, A.TOL["lengths"][name], zero=z, what=name)
