"""Output row maps of the two fused forward epilogues (vlr_gemm_qkv_rope_bias_dst, vlr_gemm_swiglu_dst): q|k|v, or act, of logical row m
is stored at destination row c_rows[m] and, where c_twin[m] >= 0, at c_twin[m] too; and the layer passes built on them
(vlr_decoder_layer_fwd_compact_maps, vlr_decoder_layer_fwd_compact_keep).  Every comparison is BITWISE; the oracle is the unmapped entry
point followed by vlr_gather_rows.  Destinations hold NaN where nothing may be written and are checked there afterwards; every case runs
twice; the launch count of the persistent kernel equals the unmapped call's.

Needs a real MI355X:  pytest -m gpu"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_hip_prefix_dedup import _acts, _rnd  # noqa: E402
from tests.test_hip_prefix_dedup_policy import (ACT_NAMES, GRAD_NAMES, _bwd_ws, _grads, _layer_setup, _plan_on_device)  # noqa: E402
from tests.test_hip_src_maps import _a_through_map, _n256, nan, same  # noqa: E402

DEV = "cuda"

# logical rows M -> (P, S) of three pairs in the proportions of build_policy_plan([1, 90, 43], 90): a pair that shares one row, an
# identical pair, a pair that shares under half - M = 6 S - sum P kept rows of 6 S dense ones
PLANS = {549: ([1, 120, 50], 120), 22100: ([1, 4800, 1899], 4800), 16700: ([1, 3640, 1499], 3640)}


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return _hip


def _maps(M):
    """-> (compact_rows [M], twin [M], dense_src [Md], Md) on the device"""
    from vlrlhf import prefix_dedup as PD
    P, S = PLANS[M]
    rows, dsrc = PD.build_row_maps(P, S)
    twin = PD.build_twin(rows, dsrc)
    Md = 6 * S
    assert rows.numel() == M and dsrc.numel() == Md and int((twin >= 0).sum()) == Md - M and int((twin < 0).sum()) > 0
    return rows.to(DEV), twin.to(DEV), dsrc.to(DEV), Md


# M = 549: three row tiles, the last partial, one tile per workgroup; 22100 / 16700: more output tiles than workgroups - pieces are
# prefetched.  K = 256: the shallowest reduction the kernels take; K = 328: a K tail on the general staging path
@pytest.mark.parametrize("a_map", [False, True], ids=["x-in-place", "x-through-a-map"])
@pytest.mark.parametrize("K", [256, 328])
@pytest.mark.parametrize("M", [549, 22100])
def test_fused_rope_stores_through_the_maps(hip, M, K, a_map):
    N, rope_cols, hd, max_pos = 768, 512, 128, 512
    cos = torch.empty(max_pos, hd // 2, dtype=torch.float32, device=DEV)
    sin = torch.empty_like(cos)
    hip.call("vlr_rope_table", cos, sin, max_pos, hd, 10000.0)
    buf, a_rows, A = _a_through_map(hip, M, K, seed=M + K)
    x, xmap = (buf, a_rows) if a_map else (A, None)
    W = _rnd(N, K, seed=3, scale=K ** -0.5)
    pos = (torch.arange(M, device=DEV) % max_pos).int()
    rows, twin, dsrc, Md = _maps(M)
    want_c = nan(M, N)
    n_ref = _n256(hip, lambda: hip.call("vlr_gemm_qkv_rope_bias", A, W, None, want_c, pos, cos, sin, M, N, rope_cols, K, K, hd, max_pos))
    want = torch.empty(Md, N, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gather_rows", want_c, dsrc, want, Md, N)
    torch.cuda.synchronize()
    assert n_ref == 1 and not bool(torch.isnan(want).any())
    for run in range(2):
        out = nan(Md + 1, N)                                    # one row behind the destination: never written
        n = _n256(hip, lambda: hip.call("vlr_gemm_qkv_rope_bias_dst", x, xmap, W, None, out, rows, twin, None, None, 0, pos, cos, sin, M, N,
                                        rope_cols, K, K, hd, max_pos))
        assert n == n_ref and same(out[:Md], want) and bool(torch.isnan(out[Md:]).all()), run
    # the twins withheld: the rows no kept row maps to are not written
    out = nan(Md + 1, N)
    hip.call("vlr_gemm_qkv_rope_bias_dst", x, xmap, W, None, out, rows, torch.full_like(twin, -1), None, None, 0, pos, cos, sin, M, N, rope_cols,
             K, K, hd, max_pos)
    torch.cuda.synchronize()
    kept = torch.zeros(Md + 1, dtype=torch.bool, device=DEV)
    kept[rows.long()] = True
    assert same(out[kept], want_c) and bool(torch.isnan(out[~kept]).all())
    with pytest.raises(ValueError, match="null output row map"):
        hip.call("vlr_gemm_qkv_rope_bias_dst", x, xmap, W, None, out, rows, None, None, None, 0, pos, cos, sin, M, N, rope_cols, K, K, hd, max_pos)


@pytest.mark.parametrize("K", [256, 328])
@pytest.mark.parametrize("M", [549, 16700])
def test_fused_swiglu_stores_act_through_the_maps(hip, M, K):
    I = 512
    buf, a_rows, A = _a_through_map(hip, M, K, seed=M + K + 1)
    W = _rnd(2 * I, K, seed=4, scale=K ** -0.5)
    rows, twin, dsrc, Md = _maps(M)
    want_gu, want_c = nan(M, 2 * I), nan(M, I)
    n_ref = _n256(hip, lambda: hip.call("vlr_gemm_swiglu", A, W, want_gu, want_c, M, I, K, K, 1))
    want = torch.empty(Md, I, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gather_rows", want_c, dsrc, want, Md, I)
    torch.cuda.synchronize()
    assert n_ref == 1 and not bool(torch.isnan(want).any())
    for run in range(2):
        gu, act = nan(M + 1, 2 * I), nan(Md + 1, I)
        n = _n256(hip, lambda: hip.call("vlr_gemm_swiglu_dst", buf, a_rows, W, gu, act, rows, twin, None, None, 0, M, I, K, K, 1))
        assert n == n_ref and same(act[:Md], want) and bool(torch.isnan(act[Md:]).all()), run
        assert same(gu[:M], want_gu) and bool(torch.isnan(gu[M:]).all()), run            # gate | up stay on the logical rows
    # store_gu = 0 (the no-grad pass): gate | up is not written; the twins withheld: the dropped rows of act are not written
    gu, act = nan(M, 2 * I), nan(Md + 1, I)
    hip.call("vlr_gemm_swiglu_dst", buf, a_rows, W, gu, act, rows, torch.full_like(twin, -1), None, None, 0, M, I, K, K, 0)
    torch.cuda.synchronize()
    kept = torch.zeros(Md + 1, dtype=torch.bool, device=DEV)
    kept[rows.long()] = True
    assert bool(torch.isnan(gu).all()) and same(act[kept], want_c) and bool(torch.isnan(act[~kept]).all())
    with pytest.raises(ValueError, match="must not be the source"):
        hip.call("vlr_gemm_swiglu_dst", buf, a_rows, W, gu, buf, rows, twin, None, None, 0, M, I, K, K, 1)


def test_fallback_is_the_unmapped_call_and_a_row_copy(hip):
    """K = 128: the fused kernel refuses the shape - the unmapped product into the fallback rows, then vlr_gather_rows; an error without them"""
    M, K, N, I, hd, max_pos = 549, 128, 768, 512, 128, 512
    cos = torch.empty(max_pos, hd // 2, dtype=torch.float32, device=DEV)
    sin = torch.empty_like(cos)
    hip.call("vlr_rope_table", cos, sin, max_pos, hd, 10000.0)
    A = _rnd(M, K, seed=9, scale=0.5)
    pos = (torch.arange(M, device=DEV) % max_pos).int()
    rows, twin, dsrc, Md = _maps(M)
    W = _rnd(N, K, seed=3, scale=K ** -0.5)
    want_c, want = nan(M, N), nan(Md, N)
    hip.call("vlr_gemm_qkv_rope_bias", A, W, None, want_c, pos, cos, sin, M, N, 512, K, K, hd, max_pos)
    hip.call("vlr_gather_rows", want_c, dsrc, want, Md, N)
    out, tmp = nan(Md + 1, N), nan(M, N)
    hip.call("vlr_gemm_qkv_rope_bias_dst", A, None, W, None, out, rows, twin, tmp, dsrc, Md, pos, cos, sin, M, N, 512, K, K, hd, max_pos)
    torch.cuda.synchronize()
    assert same(out[:Md], want) and bool(torch.isnan(out[Md:]).all())
    with pytest.raises(ValueError, match="the fallback needs"):
        hip.call("vlr_gemm_qkv_rope_bias_dst", A, None, W, None, out, rows, twin, None, None, 0, pos, cos, sin, M, N, 512, K, K, hd, max_pos)
    Wg = _rnd(2 * I, K, seed=4, scale=K ** -0.5)
    want_gu, want_c, want = nan(M, 2 * I), nan(M, I), nan(Md, I)
    hip.call("vlr_gemm_swiglu", A, Wg, want_gu, want_c, M, I, K, K, 1)
    hip.call("vlr_gather_rows", want_c, dsrc, want, Md, I)
    gu, act, tmp = nan(M, 2 * I), nan(Md + 1, I), nan(M, I)
    hip.call("vlr_gemm_swiglu_dst", A, None, Wg, gu, act, rows, twin, tmp, dsrc, Md, M, I, K, K, 1)
    torch.cuda.synchronize()
    assert same(act[:Md], want) and bool(torch.isnan(act[Md:]).all()) and same(gu, want_gu)


# ------------------------------------------------------------------------------------------------------------ one layer, C ABI
def _layer_case(hip, shape):
    if shape == "7b":
        L, Bn, S, P = _layer_setup(hip, 4096, 11008, 32, 4096, seed=60), 4, 805, [201, 201]
    else:
        L, Bn, S, P = _layer_setup(hip, 256, 512, 2, 128, seed=40), 6, 90, [1, 90, 43]
    B, M, H = Bn // 2, Bn * S, L["H"]
    km = torch.ones(Bn, S, dtype=torch.int32, device=DEV)
    pos = torch.arange(S, dtype=torch.int32, device=DEV).repeat(Bn, 1).contiguous()
    plan = _plan_on_device(hip, P, S, pos)
    x = _rnd(Bn, S, H, seed=76, dtype=torch.float32)
    for i, p in enumerate(P):
        x[B + i, :p] = x[i, :p]
    x = x.reshape(M, H).contiguous()
    xc = x[plan["compact_rows"].long()].contiguous()
    return L, Bn, S, M, km, pos, plan, x, xc


@pytest.mark.parametrize("shape", ["toy", "7b"])
def test_reference_pass_layer_with_the_maps(hip, shape):
    """vlr_decoder_layer_fwd_compact_maps (no-grad) against vlr_decoder_layer_fwd_compact: x_out on the kept rows, the dense q|k|v, the
    dense attention rows and lse; a->qkv is not written"""
    L, Bn, S, M, km, pos, plan, x, xc = _layer_case(hip, shape)
    Mc, sizes = plan["Mc"], (Bn, S, L["H"], L["I"], L["nh"], L["Nq"], L["N"])
    a0, q0, t0 = _acts(hip, Mc, *sizes), nan(M, L["N"]), nan(M, L["Nq"])
    hip.call("vlr_decoder_layer_fwd_compact", L["cfg"], L["lw"], a0["struct"], xc, plan["pos"], plan["dense_src"], plan["compact_rows"], Mc,
             plan["tail"], q0, t0, km, Bn, S)
    torch.cuda.synchronize()
    for run in range(2):
        a1, q1, t1 = _acts(hip, Mc, *sizes), nan(M + 1, L["N"]), nan(M, L["Nq"])
        hip.call("vlr_decoder_layer_fwd_compact_maps", L["cfg"], L["lw"], a1["struct"], xc, plan["struct"], q1, t1, km, Bn, S, 0)
        torch.cuda.synchronize()
        assert same(q1[:M], q0) and bool(torch.isnan(q1[M:]).all()) and same(t1, t0), run
        assert same(a1["lse"][:, :, :S], a0["lse"][:, :, :S]), run
        for n in ("xn1", "rstd1", "x_mid", "xn2", "rstd2", "act", "x_out"):
            assert same(a1[n], a0[n]), (n, run)
        assert bool(torch.isnan(a1["qkv"]).all()) and bool(torch.isnan(a1["gu"]).all()), run
    assert not bool(torch.isnan(q0).any()) and bool(torch.isfinite(a0["x_out"]).all())


@pytest.mark.parametrize("shape", ["toy", "7b"])
def test_keep_route_is_the_expand_route(hip, shape):
    """vlr_decoder_layer_fwd_compact_keep + vlr_decoder_layer_bwd_src against vlr_decoder_layer_fwd_compact_ex + vlr_layer_acts_expand +
    vlr_decoder_layer_bwd: all dense outputs, dx_in and every weight gradient bit for bit; at the 7B widths nothing is copied - the
    scratch set's xn1, qkv, xn2 and act are not written"""
    L, Bn, S, M, km, pos, plan, x, xc = _layer_case(hip, shape)
    Mc, H, I = plan["Mc"], L["H"], L["I"]
    sizes = (Bn, S, H, I, L["nh"], L["Nq"], L["N"])
    dx_out = _rnd(M, H, seed=77, scale=1e-2)
    ae, ac = _acts(hip, M, *sizes), _acts(hip, Mc, *sizes)
    sv = dict(ac, lse=ae["lse"])
    mixed = hip.LayerActs(*(sv[n].data_ptr() for n in ACT_NAMES))
    hip.call("vlr_decoder_layer_fwd_compact_ex", L["cfg"], L["lw"], mixed, xc, plan["pos"], plan["dense_src"], plan["compact_rows"], Mc,
             plan["tail"], ae["qkv"], ae["attn"], km, Bn, S, 1)
    hip.call("vlr_layer_acts_expand", L["cfg"], ac["struct"], ae["struct"], plan["dense_src"], M, 1)
    torch.cuda.synchronize()
    for run in range(2):
        ak, asc = _acts(hip, M, *sizes), _acts(hip, Mc, *sizes)
        hip.call("vlr_decoder_layer_fwd_compact_keep", L["cfg"], L["lw"], ak["struct"], asc["struct"], xc, plan["struct"], km, Bn, S)
        torch.cuda.synchronize()
        for n in ("xn1", "xn2", "act", "qkv", "attn"):
            assert same(ak[n], ae[n]), (n, run)
        assert same(ak["lse"][:, :, :S], ae["lse"][:, :, :S]), run
        for n in ("rstd1", "x_mid", "rstd2", "gu", "x_out"):
            assert same(ak[n][:Mc], ac[n]) and bool(torch.isnan(ak[n][Mc:]).all()), (n, run)
        for n in ("xn1", "qkv", "xn2") + (("act",) if shape == "7b" else ()):
            assert bool(torch.isnan(asc[n]).all()), (n, run)
    outs = []
    for route in ("expand", "src"):
        g, gs = _grads(hip, L, float("nan"))
        w, wsb = _bwd_ws(hip, M, Bn, S, L)
        dx_in = nan(M, H)
        if route == "expand":
            hip.call("vlr_decoder_layer_bwd", L["cfg"], L["lw"], gs, 0, ae["struct"], wsb, x, dx_out, dx_in, pos, km, Bn, S)
        else:
            dgu = nan(M, 2 * I)
            hip.call("vlr_decoder_layer_bwd_src", L["cfg"], L["lw"], gs, 0, ak["struct"], wsb, dgu, plan["dense_src"], xc, dx_out, dx_in, pos, km,
                     Bn, S)
        torch.cuda.synchronize()
        outs.append((dx_in, g))
    assert same(outs[1][0], outs[0][0]) and bool(torch.isfinite(outs[0][0].float()).all())
    for k in GRAD_NAMES:
        assert same(outs[1][1][k], outs[0][1][k]), k
