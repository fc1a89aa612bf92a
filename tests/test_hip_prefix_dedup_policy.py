"""The row-compact POLICY pass (engine.forward_hidden(save=True, prefix_dedup_rows=True); vlr_decoder_layer_fwd_compact_ex,
vlr_decoder_layer_bwd_compact, vlr_expand_rows_zero, vlr_fold_rows): each DPO pair's shared prompt rows are computed once in the forward
AND in the backward.  The two row kernels bit for bit against their torch restatement; one layer through the C ABI against the dense
layer and fp32 autograd, at toy widths and at the 7B widths; the trainer's step on the golden fixture; the cases in which the pass is
not taken.  Needs a real MI355X:  pytest -m gpu"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import llava_dpo_oracle as O  # noqa: E402  (checker only)
from tests.golden_util import load_case, t  # noqa: E402
from tests.test_hip_e2e import PEFT, TOL_LOSS_FP32, build, cosine, make_trainer, relmax  # noqa: E402
from tests.test_hip_prefix_dedup import _acts, _edited_batch, _rnd  # noqa: E402
from tests.test_prefix_dedup_policy_host import expand_rows_zero_ref, fold_rows_ref  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return torch.device("cuda")


# ------------------------------------------------------------------------------------------------------------ the two row kernels
@pytest.mark.parametrize("W", [8, 264, 12288])            # 12288: wider than one 8192-column sweep of the workgroup
@pytest.mark.parametrize("Mc", [1, 9])
@pytest.mark.parametrize("twins", ["none", "all", "some"])
def test_row_kernels_bit_for_bit(gpu, W, Mc, twins):
    from vlrlhf import _hip as hip
    g = torch.Generator().manual_seed(1000 * Mc + W)
    has = dict(none=torch.zeros(Mc, dtype=torch.bool), all=torch.ones(Mc, dtype=torch.bool), some=torch.arange(Mc) % 2 == 0)[twins]
    n_tw = int(has.sum())
    M = Mc + n_tw
    # a [kept ; dropped] layout like a batch's: kept rows first (ascending), the dropped twins of the marked rows after them
    rows = torch.arange(Mc, dtype=torch.int32)
    twin = torch.full((Mc,), -1, dtype=torch.int32)
    twin[has] = Mc + torch.arange(n_tw, dtype=torch.int32)
    own = torch.cat([torch.arange(Mc, dtype=torch.int32), torch.full((n_tw,), -1, dtype=torch.int32)])
    src_d = torch.randn(M, W, generator=g).bfloat16()
    src_c = torch.randn(Mc, W, generator=g).bfloat16()
    # fold: [M] -> [Mc]
    out = torch.full((Mc, W), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_fold_rows", src_d.to(DEV), rows.to(DEV), twin.to(DEV), out, Mc, W)
    torch.cuda.synchronize()
    want = fold_rows_ref(src_d, rows, twin)
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))
    # expand: [Mc] -> [M]
    out = torch.full((M, W), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_expand_rows_zero", src_c.to(DEV), own.to(DEV), out, M, W)
    torch.cuda.synchronize()
    want = expand_rows_zero_ref(src_c, own)
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))
    assert bool((out.cpu()[Mc:].view(torch.int16) == 0).all())          # +0.0, not -0.0
    # a permuted own map reads the rows it names (the engine's maps are ascending; the kernel does not rely on it)
    perm = torch.randperm(Mc, generator=g).int()
    out2 = torch.full((Mc, W), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_expand_rows_zero", src_c.to(DEV), perm.to(DEV), out2, Mc, W)
    torch.cuda.synchronize()
    assert torch.equal(out2.cpu().view(torch.int16), src_c[perm.long()].view(torch.int16))


def test_row_kernels_refuse_bad_shapes(gpu):
    from vlrlhf import _hip as hip
    x = torch.zeros(4, 16, dtype=torch.bfloat16, device=DEV)
    m = torch.zeros(4, dtype=torch.int32, device=DEV)
    for W in (0, 12):
        with pytest.raises(ValueError, match="vlr_expand_rows_zero"):
            hip.call("vlr_expand_rows_zero", x, m, x, 4, W)
        with pytest.raises(ValueError, match="vlr_fold_rows"):
            hip.call("vlr_fold_rows", x, m, m, x, 4, W)
    with pytest.raises(ValueError, match="null argument"):
        hip.call("vlr_fold_rows", x, m, None, x, 4, 16)


# ------------------------------------------------------------------------------------------------------------ one layer, C ABI
GRAD_NAMES = ("ln1", "wqkv", "wo", "ln2", "wgu", "wdown")


def _layer_setup(hip, H, I, nh, max_pos, seed):
    hd = 128
    Nq = nh * hd
    N = 3 * Nq
    cos = torch.empty(max_pos, hd // 2, dtype=torch.float32, device=DEV)
    sin = torch.empty_like(cos)
    hip.call("vlr_rope_table", cos, sin, max_pos, hd, 10000.0)
    cfg = hip.LlamaCfg(H, I, nh, hd, 1e-5, max_pos, cos.data_ptr(), sin.data_ptr(), nh, 1)
    sc = 1.0 / math.sqrt(H)
    W = dict(ln1=(1 + 0.1 * _rnd(H, seed=seed).float()).bfloat16(), wqkv=_rnd(N, H, scale=sc, seed=seed + 1), wo=_rnd(H, Nq, scale=sc, seed=seed + 2),
             ln2=(1 + 0.1 * _rnd(H, seed=seed + 3).float()).bfloat16(), wgu=_rnd(2 * I, H, scale=sc, seed=seed + 4),
             wdown=_rnd(H, I, scale=1 / math.sqrt(I), seed=seed + 5))
    lw = hip.LayerWeights(*(W[k].data_ptr() for k in GRAD_NAMES), None)
    return dict(cfg=cfg, W=W, lw=lw, keep=(cos, sin), H=H, I=I, nh=nh, Nq=Nq, N=N)


def _grads(hip, L, fill):
    g = {k: torch.full_like(L["W"][k], fill) for k in GRAD_NAMES}
    return g, hip.LayerGrads(*(g[k].data_ptr() for k in GRAD_NAMES))


def _bwd_ws(hip, rows, Bn, S, L):
    nan = lambda *s, dt=torch.bfloat16: torch.full(s, float("nan"), dtype=dt, device=DEV)      # noqa: E731
    H, I, Nq, N = L["H"], L["I"], L["Nq"], L["N"]
    w = dict(dact=nan(rows, I), dxn=nan(rows, H), dattn=nan(rows, Nq), dqkv=nan(rows, N), dx_mid=nan(rows, H),
             delta=nan(Bn, L["nh"], (S + 63) // 64 * 64, dt=torch.float32),
             norm_ws=torch.empty(hip.helper("vlr_rmsnorm_bwd_workspace_bytes", H), dtype=torch.uint8, device=DEV))
    return w, hip.LayerBwdWs(*(w[n].data_ptr() for n, _ in hip.LayerBwdWs._fields_))


def _plan_on_device(hip, P, S, pos):
    from vlrlhf import prefix_dedup as PD
    plan = PD.build_policy_plan(P, S)
    for k in ("compact_rows", "dense_src", "dense_own", "twin"):
        plan[k] = plan[k].to(DEV)
    plan["pos"] = pos.reshape(-1)[plan["compact_rows"].long()].contiguous()
    plan["struct"] = hip.RowMaps(plan["compact_rows"].data_ptr(), plan["dense_src"].data_ptr(), plan["dense_own"].data_ptr(),
                                 plan["twin"].data_ptr(), plan["pos"].data_ptr(), plan["Mc"], plan["tail"])
    return plan


def _run_dense(hip, L, x, dx_out, pos, km, Bn, S, acc, fill):
    M = Bn * S
    a = _acts(hip, M, Bn, S, L["H"], L["I"], L["nh"], L["Nq"], L["N"])
    hip.call("vlr_decoder_layer_fwd_ex", L["cfg"], L["lw"], a["struct"], x, pos, km, Bn, S, 1)
    g, gs = _grads(hip, L, fill)
    w, wsb = _bwd_ws(hip, M, Bn, S, L)
    dx_in = torch.full((M, L["H"]), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_decoder_layer_bwd", L["cfg"], L["lw"], gs, acc, a["struct"], wsb, x, dx_out, dx_in, pos, km, Bn, S)
    torch.cuda.synchronize()
    return a["x_out"].clone(), dx_in, g


def _run_compact(hip, L, plan, x, dx_out_c, km, Bn, S, acc, fill):
    M, Mc = Bn * S, plan["Mc"]
    rows = plan["compact_rows"].long()
    a = _acts(hip, Mc, Bn, S, L["H"], L["I"], L["nh"], L["Nq"], L["N"])
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.bfloat16, device=DEV)      # noqa: E731
    d = dict(qkv=nan(M, L["N"]), attn=nan(M, L["Nq"]), dattn=nan(M, L["Nq"]), dqkv=nan(M, L["N"]))
    ds = hip.DenseScratch(*(d[n].data_ptr() for n, _ in hip.DenseScratch._fields_))
    xc = x[rows].contiguous()
    hip.call("vlr_decoder_layer_fwd_compact_ex", L["cfg"], L["lw"], a["struct"], xc, plan["pos"], plan["dense_src"], plan["compact_rows"],
             Mc, plan["tail"], d["qkv"], d["attn"], km, Bn, S, 1)
    g, gs = _grads(hip, L, fill)
    w, wsb = _bwd_ws(hip, Mc, Bn, S, L)
    dx_in = torch.full((Mc, L["H"]), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_decoder_layer_bwd_compact", L["cfg"], L["lw"], gs, acc, a["struct"], wsb, plan["struct"], ds, xc, dx_out_c, dx_in, km, Bn, S)
    torch.cuda.synchronize()
    return a["x_out"].clone(), dx_in, g, dict(a=a, gs=gs, wsb=wsb, ds=ds, xc=xc, d=d)


def _oracle_layer(L, x, dx_out, pos, km, Bn, S):
    """fp32 torch autograd of the layer on the CPU (the oracle's decoder, one layer; its final norm is not read)"""
    H, I, Nq = L["H"], L["I"], L["Nq"]
    p = "language_model.model.layers.0."
    Wb = {k: v.float().cpu() for k, v in L["W"].items()}
    leaves = {k: v.clone().requires_grad_(True) for k, v in Wb.items()}
    Wo = {p + "input_layernorm.weight": leaves["ln1"], p + "self_attn.q_proj.weight": leaves["wqkv"][:Nq],
          p + "self_attn.k_proj.weight": leaves["wqkv"][Nq:2 * Nq], p + "self_attn.v_proj.weight": leaves["wqkv"][2 * Nq:],
          p + "self_attn.o_proj.weight": leaves["wo"], p + "post_attention_layernorm.weight": leaves["ln2"],
          p + "mlp.gate_proj.weight": leaves["wgu"][:I], p + "mlp.up_proj.weight": leaves["wgu"][I:], p + "mlp.down_proj.weight": leaves["wdown"],
          "language_model.model.norm.weight": torch.ones(H)}
    xe = x.float().cpu().reshape(Bn, S, H).clone().requires_grad_(True)
    out = []
    O.llama_hidden(xe, km.cpu(), pos.cpu().long(), Wo, dict(layers=1, heads=L["nh"], head_dim=128, rms_eps=1e-5), collect=out)
    x_out = out[0].reshape(Bn * S, H)
    (x_out * dx_out.float().cpu()).sum().backward()
    return x_out.detach(), xe.grad.reshape(Bn * S, H), {k: v.grad for k, v in leaves.items()}


@pytest.fixture(scope="module")
def toy_layer(gpu):
    """H = 256, 2 heads of 128, I = 512; three ragged pairs of S = 90: P = [1, S, 43] - a pair that shares one row, an identical pair,
    and a prefix off every 8-row boundary (trimmed to 41 by the plan: Mc = 408).  The fp32 autograd reference is computed once."""
    from vlrlhf import _hip as hip
    L = _layer_setup(hip, 256, 512, 2, 128, seed=40)
    B, S, P = 3, 90, [1, 90, 43]
    Bn, M, H = 2 * B, 2 * B * S, 256
    lens = torch.tensor([90, 80, 85, 70, 80, 90])
    km = (torch.arange(S)[None] < lens[:, None]).int().to(DEV).contiguous()
    pos = torch.arange(S, dtype=torch.int32, device=DEV).repeat(Bn, 1).contiguous()
    x = _rnd(Bn, S, H, seed=46, dtype=torch.float32)
    for i, p in enumerate(P):
        x[B + i, :p] = x[i, :p]
    x = x.reshape(M, H).contiguous()
    plan = _plan_on_device(hip, P, S, pos)
    assert plan["P"] == [1, 90, 41] and plan["Mc"] == 408 and plan["tail"] == 49
    dx_out_c = _rnd(plan["Mc"], H, seed=47)
    dx_out_c[(km.reshape(-1)[plan["compact_rows"].long()] == 0)] = 0           # nothing enters through a padded row
    dx_out = torch.zeros(M, H, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_expand_rows_zero", dx_out_c, plan["dense_own"], dx_out, M, H)
    torch.cuda.synchronize()
    ref = _oracle_layer(L, x, dx_out, pos, km, Bn, S)
    return dict(L=L, B=B, S=S, Bn=Bn, M=M, km=km, pos=pos, x=x, plan=plan, dx_out_c=dx_out_c, dx_out=dx_out, ref=ref)


@pytest.mark.parametrize("acc", [0, 1])
def test_compact_layer_matches_dense_and_autograd(toy_layer, acc):
    from vlrlhf import _hip as hip
    T = toy_layer
    L, plan, Bn, S, M = T["L"], T["plan"], T["Bn"], T["S"], T["M"]
    fill = 0.25 if acc else float("nan")                 # accumulate: onto a known value; else the buffers are overwritten
    xo_d, dxi_d, g_d = _run_dense(hip, L, T["x"], T["dx_out"], T["pos"], T["km"], Bn, S, acc, fill)
    xo_c, dxi_c, g_c, _ = _run_compact(hip, L, plan, T["x"], T["dx_out_c"], T["km"], Bn, S, acc, fill)
    xo32, dx32, g32 = T["ref"]
    rows, twin = plan["compact_rows"].long().cpu(), plan["twin"].long().cpu()
    valid = (T["km"].reshape(-1).cpu() != 0)
    vc = valid[rows]
    # forward: kept rows against the dense layer and against fp32 (the bound of test_hidden_states_edited_prefixes: 4e-2)
    e_cd, e_c32, e_d32 = relmax(xo_c.cpu()[vc], xo_d.cpu()[rows][vc]), relmax(xo_c.cpu()[vc], xo32[rows][vc]), relmax(xo_d.cpu()[valid], xo32[valid])
    print(f"acc {acc}: x_out kept rows compact-dense {e_cd:.3e}, compact-fp32 {e_c32:.3e}, dense-fp32 {e_d32:.3e}")
    assert e_cd < 4e-2 and e_c32 < 4e-2 and e_d32 < 4e-2
    # d x_in: a kept row's gradient is the sum over its copies
    def summed(dx):
        s = dx.float().cpu()
        out = s[rows].clone()
        has = twin >= 0
        out[has] += s[twin[has]]
        return out
    for label, got, want in (("compact-dense", dxi_c.float().cpu(), summed(dxi_d)), ("compact-fp32", dxi_c.float().cpu(), summed(dx32)),
                             ("dense-fp32", summed(dxi_d), summed(dx32))):
        cs, rm = cosine(got[vc], want[vc]), relmax(got[vc], want[vc])
        print(f"acc {acc}: dx_in {label}: cosine {cs:.5f} relmax {rm:.3e}")
        assert cs > 0.995 and rm < 8e-2, (label, cs, rm)
    assert torch.isfinite(dxi_c).all()
    # the seven weight gradients (q, k, v in wqkv; gate, up in wgu) and the two norm gradients
    for k in GRAD_NAMES:
        base = 0.25 if acc else 0.0
        for label, got, want in (("compact-fp32", g_c[k].float().cpu() - base, g32[k]), ("dense-fp32", g_d[k].float().cpu() - base, g32[k]),
                                 ("compact-dense", g_c[k].float().cpu() - base, g_d[k].float().cpu() - base)):
            cs, rm = cosine(got, want), relmax(got, want)
            print(f"acc {acc}: d {k:6s} {label}: cosine {cs:.5f} relmax {rm:.3e}")
            assert cs > 0.995 and rm < 8e-2, (k, label, cs, rm)


def test_compact_layer_argument_errors(toy_layer):
    from vlrlhf import _hip as hip
    T = toy_layer
    L, plan, Bn, S = T["L"], T["plan"], T["Bn"], T["S"]
    _, _, _, h = _run_compact(hip, L, plan, T["x"], T["dx_out_c"], T["km"], Bn, S, 0, float("nan"))
    dx_in = torch.empty(plan["Mc"], L["H"], dtype=torch.bfloat16, device=DEV)
    g, gs = _grads(hip, L, 0.0)
    null_maps = hip.RowMaps(plan["compact_rows"].data_ptr(), plan["dense_src"].data_ptr(), None, plan["twin"].data_ptr(), plan["pos"].data_ptr(),
                            plan["Mc"], plan["tail"])
    with pytest.raises(ValueError, match="null row map"):
        hip.call("vlr_decoder_layer_bwd_compact", L["cfg"], L["lw"], gs, 0, h["a"]["struct"], h["wsb"], null_maps, h["ds"], h["xc"], T["dx_out_c"],
                 dx_in, T["km"], Bn, S)
    big = hip.RowMaps(plan["compact_rows"].data_ptr(), plan["dense_src"].data_ptr(), plan["dense_own"].data_ptr(), plan["twin"].data_ptr(),
                      plan["pos"].data_ptr(), T["M"] + 1, plan["tail"])
    with pytest.raises(ValueError, match="compact rows"):
        hip.call("vlr_decoder_layer_bwd_compact", L["cfg"], L["lw"], gs, 0, h["a"]["struct"], h["wsb"], big, h["ds"], h["xc"], T["dx_out_c"],
                 dx_in, T["km"], Bn, S)
    with pytest.raises(ValueError, match="null argument"):
        hip.call("vlr_decoder_layer_bwd_compact", L["cfg"], L["lw"], gs, 0, h["a"]["struct"], h["wsb"], None, h["ds"], h["xc"], T["dx_out_c"],
                 dx_in, T["km"], Bn, S)
    with pytest.raises(ValueError, match="compact rows"):
        hip.call("vlr_decoder_layer_fwd_compact_ex", L["cfg"], L["lw"], h["a"]["struct"], h["xc"], plan["pos"], plan["dense_src"],
                 plan["compact_rows"], T["M"] + 1, 0, h["d"]["qkv"], h["d"]["attn"], T["km"], Bn, S, 1)
    assert bool((g["wo"] == 0).all())                    # nothing was launched


def test_compact_layer_true_widths(gpu):
    """ONE layer at the 7B widths (H 4096, I 11008, 32 heads) on the smallest 2-pair batch for which vlr_decoder_layer_compact_exact says
    yes, searched over S with P = S // 4 shared rows per pair: S = 805 (M = 3220 dense rows = 13 tile rows, Mc = 2824 = 12 tile rows
    after the plan kept 6 rows again; 12 x 16 = 192 tiles is the fewest the persistent kernel takes, so S = 804 with 11 tile rows is
    refused).  Forward: the kept rows are the dense layer's BIT FOR BIT.  Backward: every weight gradient against the dense layer's,
    cosine and norm ratio printed per tensor, within the bound tests/test_hip_depth.py::_check_grads applies against fp32."""
    from vlrlhf import _hip as hip
    from vlrlhf import prefix_dedup as PD
    L = _layer_setup(hip, 4096, 11008, 32, 4096, seed=60)
    found = None
    for S in range(256, 2048):
        pl = PD.build_policy_plan([S // 4] * 2, S)
        if pl["Mc"] % 8 == 0 and hip.helper("vlr_decoder_layer_compact_exact", ctypes.byref(L["cfg"]), 4, S, pl["Mc"], pl["tail"]):
            found = S
            break
    assert found == 805, found
    S, Bn, H = found, 4, 4096
    M, P = Bn * S, S // 4
    km = torch.ones(Bn, S, dtype=torch.int32, device=DEV)
    pos = torch.arange(S, dtype=torch.int32, device=DEV).repeat(Bn, 1).contiguous()
    plan = _plan_on_device(hip, [P, P], S, pos)
    assert (M, plan["Mc"], plan["P"]) == (3220, 2824, [201, 195])
    x = _rnd(Bn, S, H, seed=66, dtype=torch.float32)
    x[2:, :P] = x[:2, :P]
    x = x.reshape(M, H).contiguous()
    dx_out_c = _rnd(plan["Mc"], H, seed=67, scale=1e-2)
    dx_out = torch.zeros(M, H, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_expand_rows_zero", dx_out_c, plan["dense_own"], dx_out, M, H)
    xo_d, dxi_d, g_d = _run_dense(hip, L, x, dx_out, pos, km, Bn, S, 0, float("nan"))
    xo_c, dxi_c, g_c, _ = _run_compact(hip, L, plan, x, dx_out_c, km, Bn, S, 0, float("nan"))
    rows = plan["compact_rows"].long()
    assert torch.isfinite(xo_c).all() and torch.equal(xo_c, xo_d[rows])
    for k in GRAD_NAMES:
        a, b = g_c[k].float().reshape(-1), g_d[k].float().reshape(-1)
        cs = float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-30))
        nr = abs(float(a.double().norm()) / float(b.double().norm()) - 1.0)
        rm = float((a - b).abs().max()) / (float(b.abs().max()) + 1e-12)
        print(f"7B widths, d {k:6s} compact vs dense: cosine {cs:.6f} relmax {rm:.3e} norm deviation {nr:.2e}")
        assert torch.isfinite(a).all() and cs > 0.99 and nr < 0.03, (k, cs, nr)


ACT_NAMES = ("xn1", "rstd1", "qkv", "attn", "lse", "x_mid", "xn2", "rstd2", "gu", "act", "x_out")


@pytest.mark.parametrize("shape", ["toy", "7b"])
def test_expanded_activations_feed_the_dense_backward(gpu, shape):
    """compact forward + vlr_layer_acts_expand = what the dense backward reads.  At the 7B widths (the exact shape of
    test_compact_layer_true_widths: S = 805) all eleven tensors are the dense forward's BIT FOR BIT, so the unchanged dense backward
    on them gives the dense step's gradients bit for bit; at the toy widths (the GEMM route depends on the row count) the dropped rows
    are copies of their twins and the kept rows answer to the bound of the forward."""
    from vlrlhf import _hip as hip
    if shape == "7b":
        L, Bn, S, P = _layer_setup(hip, 4096, 11008, 32, 4096, seed=60), 4, 805, [201, 201]
    else:
        L, Bn, S, P = _layer_setup(hip, 256, 512, 2, 128, seed=40), 6, 90, [1, 90, 43]
    B, M, H = Bn // 2, Bn * S, L["H"]
    km = torch.ones(Bn, S, dtype=torch.int32, device=DEV)
    pos = torch.arange(S, dtype=torch.int32, device=DEV).repeat(Bn, 1).contiguous()
    plan = _plan_on_device(hip, P, S, pos)
    Mc = plan["Mc"]
    exact = bool(hip.helper("vlr_decoder_layer_compact_exact", ctypes.byref(L["cfg"]), Bn, S, Mc, plan["tail"]))
    assert exact == (shape == "7b")
    x = _rnd(Bn, S, H, seed=76, dtype=torch.float32)
    for i, p in enumerate(P):
        x[B + i, :p] = x[i, :p]
    x = x.reshape(M, H).contiguous()
    ad = _acts(hip, M, Bn, S, H, L["I"], L["nh"], L["Nq"], L["N"])
    hip.call("vlr_decoder_layer_fwd_ex", L["cfg"], L["lw"], ad["struct"], x, pos, km, Bn, S, 1)
    ae = _acts(hip, M, Bn, S, H, L["I"], L["nh"], L["Nq"], L["N"])          # the expanded set, NaN-poisoned
    ac = _acts(hip, Mc, Bn, S, H, L["I"], L["nh"], L["Nq"], L["N"])
    sv = dict(ac, lse=ae["lse"])
    mixed = hip.LayerActs(*(sv[n].data_ptr() for n in ACT_NAMES))
    xc = x[plan["compact_rows"].long()].contiguous()
    hip.call("vlr_decoder_layer_fwd_compact_ex", L["cfg"], L["lw"], mixed, xc, plan["pos"], plan["dense_src"], plan["compact_rows"], Mc,
             plan["tail"], ae["qkv"], ae["attn"], km, Bn, S, 1)
    hip.call("vlr_layer_acts_expand", L["cfg"], ac["struct"], ae["struct"], plan["dense_src"], M, 1)
    torch.cuda.synchronize()
    dsrc = plan["dense_src"].long()
    for n in ACT_NAMES:
        got, want = ae[n], ad[n]
        if n == "lse":
            got, want = got[:, :, :S], want[:, :, :S]
        assert torch.isfinite(got).all(), n
        if n != "lse" and n != "qkv" and n != "attn":
            assert torch.equal(got, ac[n][dsrc]), n                            # every dense row is its source row
        if exact:
            assert torch.equal(got, want), n
        else:
            assert relmax(got, want) < 4e-2, (n, relmax(got, want))
    if exact:                                                                  # ... and so the dense backward gives the same bits
        dx_out = _rnd(M, H, seed=77, scale=1e-2)
        outs = []
        for a in (ad, ae):
            g, gs = _grads(hip, L, float("nan"))
            w, wsb = _bwd_ws(hip, M, Bn, S, L)
            dx_in = torch.full((M, H), float("nan"), dtype=torch.bfloat16, device=DEV)
            hip.call("vlr_decoder_layer_bwd", L["cfg"], L["lw"], gs, 0, a["struct"], wsb, x, dx_out, dx_in, pos, km, Bn, S)
            torch.cuda.synchronize()
            outs.append((dx_in, g))
        assert torch.equal(outs[0][0], outs[1][0]) and all(torch.equal(outs[0][1][k], outs[1][1][k]) for k in GRAD_NAMES)
    with pytest.raises(ValueError, match="vlr_layer_acts_expand"):
        hip.call("vlr_layer_acts_expand", L["cfg"], ac["struct"], ae["struct"], None, M, 1)


# ------------------------------------------------------------------------------------------------------------ the trainer's step
def _step(cfg, W, W_ref, batch, ckpt=False, steps=1, setup=None, bwd=True, **kw):
    """a fresh model, `steps` micro-steps of the trainer -> (last loss, gradient buffer, engine, model); bwd: the backward runs on
    the kept rows too (engine.prefix_dedup_policy_backward; its default, False, is the dense backward on expanded activations)"""
    model, ref = build(cfg, W, W_ref)
    tr = make_trainer(model, None if "peft_config" in kw else ref, cfg, **kw)
    eng = model.engine
    assert eng.prefix_dedup_policy and eng.prefix_dedup_policy_exact_only and not eng.prefix_dedup_policy_backward      # the defaults
    eng.prefix_dedup_min_share = 0.0
    eng.prefix_dedup_policy_exact_only = False
    eng.prefix_dedup_policy_backward = bwd
    if setup is not None:
        setup(eng)
    if ckpt:
        model.gradient_checkpointing_enable()
    model.train()
    for _ in range(steps):
        loss = tr.training_step(model, dict(batch))
    torch.cuda.synchronize()
    g = eng.lora_grads if "peft_config" in kw else eng.grads
    return float(loss), g.clone(), eng, model


@pytest.fixture(scope="module")
def golden_steps(gpu):
    """the steps several tests compare, run once: compact (twice), compact under gradient checkpointing, dense by the switch"""
    z, cfg, W, W_ref, batch, rows = load_case("llava_hipsmall")
    case = (cfg, W, W_ref, batch)
    return dict(z=z, case=case, on=_step(*case), on2=_step(*case), ckpt=_step(*case, ckpt=True),
                off=_step(*case, setup=lambda e: setattr(e, "prefix_dedup_policy", False)))


def test_golden_step_compact_policy(golden_steps):
    z = golden_steps["z"]
    loss, grads, eng, model = golden_steps["on"]
    assert eng.prefix_dedup_policy_passes == 1 and eng.prefix_dedup_passes == 1
    d = eng.last_prefix_dedup_policy
    assert d["Mc"] % 8 == 0 and d["Mc"] == d["M"] - sum(d["P"]) and d["exact"] is False and d["backward"] == "compact", d    # toy widths: never the exact route
    exp = float(z["loss_mean_sigmoid"])
    print(f"compact policy step: loss {loss:.6f} golden {exp:.6f}; rows {d['Mc']} of {d['M']}, P {d['P']}")
    assert abs(loss - exp) < TOL_LOSS_FP32, (loss, exp)
    named = dict(model.named_parameters())
    n = 0
    for k in z.files:
        if k.startswith("grad."):
            g, want = named[k[5:]].grad, t(z, k)
            cs, rm = cosine(g, want), relmax(g, want)
            assert cs > 0.995 and rm < 8e-2, (k, cs, rm)
            n += 1
    assert n == len(named)
    # the same bits twice, and under gradient checkpointing
    for other in ("on2", "ckpt"):
        l2, g2, e2, _ = golden_steps[other]
        assert e2.prefix_dedup_policy_passes == 1
        assert l2 == loss and torch.equal(g2, grads), other
    # switched off, the step is the step of the defaults (exact-only: the toy shape runs dense), bit for bit
    l_off, g_off, e_off, _ = golden_steps["off"]
    cfg, W, W_ref, batch = golden_steps["case"]
    l_def, g_def, e_def, _ = _step(cfg, W, W_ref, batch, setup=lambda e: setattr(e, "prefix_dedup_policy_exact_only", True))
    assert e_off.prefix_dedup_policy_passes == 0 and e_def.prefix_dedup_policy_passes == 0 and e_off.prefix_dedup_passes == 1
    assert l_off == l_def and torch.equal(g_off, g_def)
    print(f"compact vs dense step: loss {loss:.6f} / {l_off:.6f}, gradient cosine {cosine(grads, g_off):.6f} relmax {relmax(grads, g_off):.3e}")


def test_golden_step_compact_forward_dense_backward(golden_steps):
    """the default route (prefix_dedup_policy_backward = False): the forward on the kept rows, the unchanged dense backward on the
    expanded activations.  Same bounds against the golden step; two runs the same bits; under gradient checkpointing (the recompute
    is the dense layer forward, which at these toy widths takes another GEMM route than the compact one) the bounds again."""
    z = golden_steps["z"]
    cfg, W, W_ref, batch = golden_steps["case"]
    exp = float(z["loss_mean_sigmoid"])
    runs = [_step(cfg, W, W_ref, batch, bwd=False), _step(cfg, W, W_ref, batch, bwd=False), _step(cfg, W, W_ref, batch, bwd=False, ckpt=True)]
    for loss, grads, eng, model in runs:
        d = eng.last_prefix_dedup_policy
        assert eng.prefix_dedup_policy_passes == 1 and eng.prefix_dedup_passes == 1 and d["backward"] == "dense", d
        assert abs(loss - exp) < TOL_LOSS_FP32, (loss, exp)
        named = dict(model.named_parameters())
        for k in z.files:
            if k.startswith("grad."):
                cs, rm = cosine(named[k[5:]].grad, t(z, k)), relmax(named[k[5:]].grad, t(z, k))
                assert cs > 0.995 and rm < 8e-2, (k, cs, rm)
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    l_off, g_off, _, _ = golden_steps["off"]
    print(f"compact forward + dense backward vs dense step: loss {runs[0][0]:.6f} / {l_off:.6f}, gradient cosine "
          f"{cosine(runs[0][1], g_off):.6f} relmax {relmax(runs[0][1], g_off):.3e}")


def test_golden_second_micro_step_accumulates(golden_steps):
    cfg, W, W_ref, batch = golden_steps["case"]
    _, g1, _, _ = golden_steps["on"]
    _, g2, eng, _ = _step(cfg, W, W_ref, batch, steps=2)
    assert eng.prefix_dedup_policy_passes == 2
    assert relmax(g2.float(), 2 * g1.float()) < 2e-2          # the bound of test_second_step_and_grad_accumulation


def test_identical_pair_against_oracle(gpu):
    """pair 1 of the batch is identical (P = S): its labelled rows are shared rows, d hidden arrives on both copies and is folded"""
    z, cfg, W, W_ref, _, _ = load_case("llava_hipsmall")
    batch, _ = _edited_batch(cfg)
    loss, grads, eng, model = _step(cfg, W, W_ref, batch)
    assert eng.prefix_dedup_policy_passes == 1
    S = eng.last_prefix_dedup_policy["M"] // 6
    assert eng.last_prefix_dedup_policy["P"][1] == S
    Wg = {k: v.bfloat16().float().requires_grad_(not k.startswith("vision_tower.")) for k, v in W.items()}
    l32, _ = O.compute_loss(Wg, {k: v.bfloat16().float() for k, v in W_ref.items()}, cfg, batch, cfg["beta"])
    l32.backward()
    assert abs(loss - float(l32)) < TOL_LOSS_FP32, (loss, float(l32))
    named = dict(model.named_parameters())
    for name, p in named.items():
        if Wg[name].grad is None:            # the frozen vision tower
            continue
        cs, rm = cosine(p.grad, Wg[name].grad), relmax(p.grad, Wg[name].grad)
        assert cs > 0.995 and rm < 8e-2, (name, cs, rm)


# ------------------------------------------------------------------------------------------------------------ not taken
def _off(e):
    e.prefix_dedup_policy = False


@pytest.mark.parametrize("case", ["lora", "neftune", "min_share"])
def test_not_taken_steps_are_dense(gpu, case):
    z, cfg, W, W_ref, batch, rows = load_case("llava_hipsmall")
    kw = dict(peft_config=dict(PEFT)) if case == "lora" else {}

    def setup(e):
        if case == "neftune":
            e.set_neftune(5.0, seed=3)
        if case == "min_share":
            e.prefix_dedup_min_share = 0.99

    def setup_off(e):
        setup(e)
        _off(e)
    l1, g1, e1, _ = _step(cfg, W, W_ref, batch, setup=setup, **kw)
    l0, g0, e0, _ = _step(cfg, W, W_ref, batch, setup=setup_off, **kw)
    assert e1.prefix_dedup_policy_passes == 0 and e0.prefix_dedup_policy_passes == 0 and e1.last_prefix_dedup_policy is None
    assert l1 == l0 and torch.equal(g1, g0)
    assert float(g1.float().abs().sum()) > 0


def test_not_taken_forwards_are_dense(gpu):
    """a no-grad policy forward inside policy_pass(), and a training forward whose images are not two identical halves (image_dup == 1)"""
    z, cfg, W, W_ref, batch, rows = load_case("llava_hipsmall")
    model, ref = build(cfg, W, W_ref)
    tr = make_trainer(model, ref, cfg)
    eng = model.engine
    eng.prefix_dedup_min_share, eng.prefix_dedup_policy_exact_only = 0.0, False
    model.train()
    outs = []
    for on in (True, False):
        eng.prefix_dedup_policy = on
        with torch.no_grad(), model.policy_pass():
            pc, pr, _, _ = tr.concatenated_forward(model, dict(batch))
        outs.append(torch.cat([pc, pr]).float().cpu())
    assert eng.prefix_dedup_policy_passes == 0 and eng.prefix_dedup_passes == 0
    assert torch.equal(outs[0], outs[1])
    cb = tr.concatenated_inputs(dict(batch), device=gpu)
    img = dict(cb["concatenated_img_input_dict"])
    img["pixel_values"] = img["pixel_values"].clone()              # the copy does not say that its halves are equal
    assert getattr(img["pixel_values"], "_vlr_dup", 1) == 1
    hid = []
    for on in (True, False):
        eng.prefix_dedup_policy = on
        with model.policy_pass():
            out = model(input_ids=cb["concatenated_input_ids"], attention_mask=cb["concatenated_attention_mask"],
                        labels=cb["concatenated_labels"], use_cache=False, **img)
        assert out.logits.c["plan"] is None and out.logits.c["acts"] is not None
        hid.append(out.logits.c["hidden"].clone())
    torch.cuda.synchronize()
    assert eng.prefix_dedup_policy_passes == 0
    assert torch.equal(hid[0], hid[1])
    # ... while the same training forward with the doubled images takes it
    eng.prefix_dedup_policy = True
    with model.policy_pass():
        out = model(input_ids=cb["concatenated_input_ids"], attention_mask=cb["concatenated_attention_mask"],
                    labels=cb["concatenated_labels"], use_cache=False, **cb["concatenated_img_input_dict"])
    assert eng.prefix_dedup_policy_passes == 1 and eng.last_prefix_dedup_policy["backward"] == "dense" and out.logits.c["plan"] is None
    eng.prefix_dedup_policy_backward = True
    with model.policy_pass():
        out = model(input_ids=cb["concatenated_input_ids"], attention_mask=cb["concatenated_attention_mask"],
                    labels=cb["concatenated_labels"], use_cache=False, **cb["concatenated_img_input_dict"])
    assert eng.prefix_dedup_policy_passes == 2 and out.logits.c["plan"] is not None
    assert tuple(out.logits.c["hidden"].shape) == tuple(hid[0].shape)
