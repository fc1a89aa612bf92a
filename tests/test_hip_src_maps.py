"""The dense policy backward on the kept rows IN PLACE: vlr_rmsnorm_bwd_src / _f32_src, vlr_gemm_swiglu_bwd_src (fused epilogue,
ring and per-row bodies, and the unfused fallback vlr_swiglu_bwd_src), vlr_decoder_layer_fwd_compact_keep +
vlr_decoder_layer_bwd_src, and the trainer's default route over them; the forward's side of it: vlr_rmsnorm_fwd_scatter / _f32_scatter
and the M-side row map on the A operand of the fused q|k|v + RoPE, fused gate|up + SwiGLU and residual-projection launches
(vlr_gemm_qkv_rope_bias_rows, vlr_gemm_swiglu_rows, vlr_gemm_res_rows).  Every comparison is BITWISE; the oracle is the unmapped
kernel on a buffer that vlr_gather_rows / vlr_gather_f32 expanded.  Buffers hold NaN where nothing may be written and are checked
there afterwards; every case runs twice; every map is valid.

Not reachable, so not covered: the one-tile-per-workgroup TAIL launch of the fused SwiGLU backward.  choose_peel prices a peeled tile
row of a fused epilogue at 1.15 rounds, and removing k rounds' worth of tiles from the main launch saves at most k rounds, so the
peel is never chosen - for vlr_gemm_swiglu_bwd and for its _src form alike (the code mirrors the unmapped entry point's).

Needs a real MI355X:  pytest -m gpu"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.golden_util import load_case  # noqa: E402
from tests.test_hip_prefix_dedup import _acts, _rnd  # noqa: E402
from tests.test_hip_prefix_dedup_policy import (ACT_NAMES, GRAD_NAMES, _bwd_ws, _grads, _layer_setup, _plan_on_device,  # noqa: E402
                                                _step)

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return _hip


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def nan(*shape, dt=torch.bfloat16):
    return torch.full(shape, NAN, dtype=dt, device=DEV)


def _maps(M):
    """name -> (src_rows [M] int32 on the CPU, Mc): identity; the duplicating map of a policy plan (M = 540: P = [1, 90, 43] at
    S = 90) or its shape by hand (a prefix read twice); duplicates `M // 2 + 3` rows apart - above the grid of 1024 workgroups the
    two readers of a source row sit in different workgroups' row walks (their distance is no multiple of 1024)"""
    out = {"identity": (torch.arange(M, dtype=torch.int32), M)}
    if M == 540:
        from vlrlhf import prefix_dedup as PD
        plan = PD.build_policy_plan([1, 90, 43], 90)
        assert plan["M"] == M
        out["plan"] = (plan["dense_src"].int().cpu(), plan["Mc"])
    else:
        h, p = M // 2, M // 5
        out["prefix"] = (torch.cat([torch.arange(h), torch.arange(p), torch.arange(h, M - p)]).int(), M - p)
    far = M // 2 + 3
    out["far"] = ((torch.arange(M) % far).int(), far)
    return out


# ------------------------------------------------------------------------------------------------------------ RMSNorm backward
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("M", [37, 540, 1037])           # 1037: above the grid of 1024 workgroups - a workgroup walks two rows
@pytest.mark.parametrize("H", [256, 4096, 5120])         # register window 2 (H <= 4096) and 4
def test_norm_backward_reads_through_the_map(hip, H, M, f32):
    entry = "vlr_rmsnorm_bwd_f32" if f32 else "vlr_rmsnorm_bwd"
    ws = torch.empty(hip.helper("vlr_rmsnorm_bwd_workspace_bytes", H), dtype=torch.uint8, device=DEV)
    dy = _rnd(M, H, seed=H + M, scale=1e-2)
    dres = _rnd(M, H, seed=H + M + 1, scale=1e-2)
    w = (1 + 0.1 * _rnd(H, seed=5).float()).bfloat16()
    dw0 = _rnd(H, seed=6)
    for name, (src, Mc) in _maps(M).items():
        src = src.to(DEV)
        assert int(src.min()) >= 0 and int(src.max()) < Mc
        pad = 3                                                # rows behind the kept rows: never read (NaN would reach dx / dw)
        x = nan(Mc + pad, H, dt=torch.float32 if f32 else torch.bfloat16)
        x[:Mc] = _rnd(Mc, H, seed=7, dtype=x.dtype)
        rstd = nan(Mc + pad, dt=torch.float32)
        rstd[:Mc] = torch.rand(Mc, device=DEV) + 0.5
        x0, rstd0 = x.clone(), rstd.clone()
        # the oracle's inputs: the library's own row copies
        xe = torch.empty(M, H, dtype=x.dtype, device=DEV)
        hip.call("vlr_gather_rows", x, src, xe, M, H * (2 if f32 else 1))
        re_ = torch.empty(M, dtype=torch.float32, device=DEV)
        hip.call("vlr_gather_f32", rstd, src, re_, M)
        for use_res, acc in ((False, 0), (True, 0), (True, 1)):
            r = dres if use_res else None
            want_dx, want_dw = nan(M, H), dw0.clone()
            hip.call(entry, dy, xe, w, re_, r, want_dx, want_dw, acc, ws, M, H)
            torch.cuda.synchronize()
            for run in range(2):
                dx = nan(M + 1, H)
                dw = dw0.clone()
                hip.call(entry + "_src", dy, x, w, rstd, r, dx, dw, acc, ws, src, M, H)
                torch.cuda.synchronize()
                tag = (name, use_res, acc, run)
                assert same(dx[:M], want_dx), tag
                assert same(dw, want_dw), tag
                assert bool(torch.isnan(dx[M:]).all()), tag                  # nothing behind the last row
                assert same(x, x0) and same(rstd, rstd0), tag               # the kept rows are read only
            # no weight gradient asked for: dx alone
            dx = nan(M, H)
            hip.call(entry + "_src", dy, x, w, rstd, r, dx, None, 0, ws, src, M, H)
            torch.cuda.synchronize()
            assert same(dx, want_dx), (name, "no dw")
    with pytest.raises(ValueError, match="null row map"):
        hip.call(entry + "_src", dy, xe, w, re_, None, want_dx, None, 0, ws, None, M, H)


# ------------------------------------------------------------------------------------------------------------ SwiGLU backward
def _swiglu_maps(M):
    """identity; a prefix read twice with both jumps inside the second row tile (rows 256 .. 511: a straddling tile between a fully
    contiguous first tile and contiguous later ones; with M = 549 the last tile is partial); the same with the jumps in the LAST,
    partial tile; and a map that is contiguous from row to row nowhere (every wave takes the per-row body)"""
    out = {"identity": (torch.arange(M, dtype=torch.int32), M)}
    if M > 512:
        a, p = 300, 70
        out["straddle"] = (torch.cat([torch.arange(a), torch.arange(p), torch.arange(a, M - p)]).int(), M - p)
        a, p = 520, 11
        out["straddle-last"] = (torch.cat([torch.arange(a), torch.arange(p), torch.arange(a, M - p)]).int(), M - p)
    g = torch.Generator().manual_seed(M)
    Mc = max(8, M // 2)
    out["scattered"] = (torch.randint(0, Mc, (M,), generator=g).int(), Mc)
    return out


SWIGLU_SHAPES = [
    # (M, I, H, fused): H = 256 = four K tiles is the shallowest reduction the persistent kernel takes; I = 512 is two column tiles,
    # I = 520 leaves 8 columns in a third; M = 549 = two full row tiles and 37 rows; H = 128: refused - plain GEMM + vlr_swiglu_bwd_src
    (549, 512, 256, True), (549, 520, 256, True), (37, 512, 256, True), (549, 520, 128, False), (37, 512, 128, False),
]


@pytest.mark.parametrize("M,I,H,fused", SWIGLU_SHAPES, ids=[f"{m}x{i}x{h}" for m, i, h, _ in SWIGLU_SHAPES])
def test_swiglu_backward_reads_through_the_map(hip, M, I, H, fused):
    dy = _rnd(M, H, seed=M + I, scale=0.5)
    wdown = _rnd(H, I, seed=M + I + 1, scale=H ** -0.5)
    for name, (src, Mc) in _swiglu_maps(M).items():
        src = src.to(DEV)
        assert int(src.min()) >= 0 and int(src.max()) < Mc
        gu = nan(Mc + 2, 2 * I)                               # two rows behind the kept rows: never read
        gu[:Mc] = _rnd(Mc, 2 * I, seed=11)
        gu0 = gu.clone()
        want = torch.empty(M, 2 * I, dtype=torch.bfloat16, device=DEV)
        hip.call("vlr_gather_rows", gu, src, want, M, 2 * I)
        hip.lib_profile_start(1)
        hip.call("vlr_gemm_swiglu_bwd", dy, wdown, want, nan(M, I), M, I, H)
        n_ref = hip.lib_profile_stop()["gemm256p"][0]
        torch.cuda.synchronize()
        assert not bool(torch.isnan(want).any())
        for run in range(2):
            out = nan(M + 2, 2 * I)
            hip.lib_profile_start(1)
            hip.call("vlr_gemm_swiglu_bwd_src", dy, wdown, gu, src, out, nan(M, I), M, I, H)
            n256 = hip.lib_profile_stop()["gemm256p"][0]
            torch.cuda.synchronize()
            tag = (name, run)
            # the route: one launch of the persistent kernel where the unmapped entry point launches one, none where it launches none
            assert n256 == n_ref == (1 if fused else 0), (tag, n256, n_ref)
            assert same(out[:M], want), tag
            assert bool(torch.isnan(out[M:]).all()), tag
            assert same(gu, gu0), tag                                        # gate | up stay the forward's
    with pytest.raises(ValueError, match="must not alias"):
        hip.call("vlr_gemm_swiglu_bwd_src", dy, wdown, gu, src, gu, nan(M, I), M, I, H)


# ------------------------------------------------------------------------------------------------------------ one layer, C ABI
@pytest.mark.parametrize("shape", ["toy", "7b"])
def test_layer_backward_in_place_is_the_expand_route(hip, shape):
    """vlr_decoder_layer_fwd_compact_keep + vlr_decoder_layer_bwd_src against vlr_decoder_layer_fwd_compact_ex +
    vlr_layer_acts_expand + vlr_decoder_layer_bwd: dx_in and every weight gradient the same bits, overwrite and accumulate"""
    if shape == "7b":
        L, Bn, S, P = _layer_setup(hip, 4096, 11008, 32, 4096, seed=60), 4, 805, [201, 201]
    else:
        L, Bn, S, P = _layer_setup(hip, 256, 512, 2, 128, seed=40), 6, 90, [1, 90, 43]
    B, M, H, I = Bn // 2, Bn * S, L["H"], L["I"]
    km = torch.ones(Bn, S, dtype=torch.int32, device=DEV)
    pos = torch.arange(S, dtype=torch.int32, device=DEV).repeat(Bn, 1).contiguous()
    plan = _plan_on_device(hip, P, S, pos)
    Mc = plan["Mc"]
    x = _rnd(Bn, S, H, seed=76, dtype=torch.float32)
    for i, p in enumerate(P):
        x[B + i, :p] = x[i, :p]
    x = x.reshape(M, H).contiguous()
    xc = x[plan["compact_rows"].long()].contiguous()
    dx_out = _rnd(M, H, seed=77, scale=1e-2)
    sizes = (M, Bn, S, H, I, L["nh"], L["Nq"], L["N"])
    # the expand route
    ae, ac = _acts(hip, *sizes), _acts(hip, Mc, *sizes[1:])
    sv = dict(ac, lse=ae["lse"])
    mixed = hip.LayerActs(*(sv[n].data_ptr() for n in ACT_NAMES))
    hip.call("vlr_decoder_layer_fwd_compact_ex", L["cfg"], L["lw"], mixed, xc, plan["pos"], plan["dense_src"], plan["compact_rows"], Mc,
             plan["tail"], ae["qkv"], ae["attn"], km, Bn, S, 1)
    hip.call("vlr_layer_acts_expand", L["cfg"], ac["struct"], ae["struct"], plan["dense_src"], M, 1)
    # the new forward: the layer's own set NaN behind the kept rows of what stays compact, the scratch set Mc rows
    ak, asc = _acts(hip, *sizes), _acts(hip, Mc, *sizes[1:])
    hip.call("vlr_decoder_layer_fwd_compact_keep", L["cfg"], L["lw"], ak["struct"], asc["struct"], xc, plan["struct"], km, Bn, S)
    torch.cuda.synchronize()
    for n in ("xn1", "xn2", "act", "qkv", "attn"):
        assert same(ak[n], ae[n]), n                                          # dense, as the expand route leaves them
    assert same(ak["lse"][:, :, :S], ae["lse"][:, :, :S])
    for n in ("rstd1", "x_mid", "rstd2", "gu", "x_out"):
        assert same(ak[n][:Mc], ac[n]), n                                     # the kept rows, in place
        assert bool(torch.isnan(ak[n][Mc:]).all()), n                         # ... and nothing behind them
    keep0 = {n: ak[n].clone() for n in ACT_NAMES}
    for acc in (0, 1):
        outs = []
        for route in ("expand", "src", "src"):
            g, gs = _grads(hip, L, 0.25 if acc else NAN)
            w, wsb = _bwd_ws(hip, M, Bn, S, L)
            dx_in = nan(M, H)
            if route == "expand":
                a2 = {n: ae[n].clone() for n in ACT_NAMES}                    # (the dense backward overwrites gate | up)
                st = hip.LayerActs(*(a2[n].data_ptr() for n in ACT_NAMES))
                hip.call("vlr_decoder_layer_bwd", L["cfg"], L["lw"], gs, acc, st, wsb, x, dx_out, dx_in, pos, km, Bn, S)
            else:
                dgu = nan(M + 1, 2 * I)
                hip.call("vlr_decoder_layer_bwd_src", L["cfg"], L["lw"], gs, acc, ak["struct"], wsb, dgu, plan["dense_src"], xc, dx_out, dx_in,
                         pos, km, Bn, S)
                torch.cuda.synchronize()
                assert bool(torch.isnan(dgu[M:]).all()) and not bool(torch.isnan(dgu[:M]).any())
                for n in ACT_NAMES:
                    assert same(ak[n], keep0[n]), n                           # the backward writes none of the kept activations
            torch.cuda.synchronize()
            outs.append((dx_in, g, w["dqkv"]))
        for o in outs[1:]:
            assert same(o[0], outs[0][0]), acc
            assert same(o[2], outs[0][2]), acc                                # d qkv, whose column sum is a q|k|v bias gradient
            for k in GRAD_NAMES:
                assert same(o[1][k], outs[0][1][k]), (acc, k)
        assert bool(torch.isfinite(outs[0][0].float()).all())


# ------------------------------------------------------------------------------------------------------------ the trainer's step
def test_trainer_step_in_place_is_the_expand_step(hip):
    """llava_hipsmall, prefix_dedup_policy_exact_only = False: the default route (kept rows read in place) against the expand route
    (engine.prefix_dedup_policy_expand): loss and the gradient buffer bit for bit, twice, and over two accumulating micro-steps"""
    z, cfg, W, W_ref, batch, rows = load_case("llava_hipsmall")
    seen = {}

    def expand(e):
        assert e.prefix_dedup_policy_expand is False          # the default: in place
        e.prefix_dedup_policy_expand = True

    def spy(e):
        fwd = e._forward_layers_compact_keep

        def wrapped(*a, **k):
            seen["keep"] = seen.get("keep", 0) + 1
            return fwd(*a, **k)
        e._forward_layers_compact_keep = wrapped

    for steps in (1, 2):
        seen.clear()
        l_new, g_new, e_new, _ = _step(cfg, W, W_ref, batch, bwd=False, steps=steps, setup=spy)
        l_new2, g_new2, _, _ = _step(cfg, W, W_ref, batch, bwd=False, steps=steps)
        l_exp, g_exp, e_exp, _ = _step(cfg, W, W_ref, batch, bwd=False, steps=steps, setup=expand)
        assert seen.get("keep") == steps                      # the default route IS the in-place one
        for e in (e_new, e_exp):
            d = e.last_prefix_dedup_policy
            assert e.prefix_dedup_policy_passes == steps and e.prefix_dedup_passes == steps and d["backward"] == "dense", d
            assert d["Mc"] % 8 == 0 and d["Mc"] == d["M"] - sum(d["P"])
        assert l_new == l_exp == l_new2, (l_new, l_exp, l_new2)
        assert same(g_new, g_exp) and same(g_new, g_new2), steps
        assert float(g_new.float().abs().sum()) > 0 and bool(torch.isfinite(g_new.float()).all())


def test_context_of_the_in_place_route(hip):
    """ctx["plan"] stays None (the backward is dense), ctx["src_plan"] names the maps; under gradient checkpointing the expand route runs"""
    from tests.test_hip_e2e import build, make_trainer
    z, cfg, W, W_ref, batch, rows = load_case("llava_hipsmall")
    model, ref = build(cfg, W, W_ref)
    tr = make_trainer(model, ref, cfg)
    eng = model.engine
    eng.prefix_dedup_min_share, eng.prefix_dedup_policy_exact_only = 0.0, False
    model.train()
    cb = tr.concatenated_inputs(dict(batch), device=torch.device(DEV))

    def fwd():
        with model.policy_pass():
            return model(input_ids=cb["concatenated_input_ids"], attention_mask=cb["concatenated_attention_mask"],
                         labels=cb["concatenated_labels"], use_cache=False, **cb["concatenated_img_input_dict"]).logits.c
    c = fwd()
    assert c["plan"] is None and c["src_plan"] is not None and eng.last_prefix_dedup_policy["backward"] == "dense"
    Mc, M = c["src_plan"]["Mc"], c["M"]
    assert tuple(c["hidden"].shape) == (M, eng.H) and c["x0_c"] is not None and len(c["acts"]) == eng.L
    hidden = c["hidden"].clone()
    eng.prefix_dedup_policy_expand = True
    c2 = fwd()
    assert c2["plan"] is None and c2["src_plan"] is None
    assert same(c2["hidden"], hidden)                         # the same forward, bit for bit
    eng.prefix_dedup_policy_expand = False
    model.gradient_checkpointing_enable()
    c3 = fwd()
    assert c3["plan"] is None and c3["src_plan"] is None and c3["ckpt"]
    torch.cuda.synchronize()
    assert eng.prefix_dedup_policy_passes == 3


# ------------------------------------------------------------------------------------------------------------ scatter norm forward
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("H", [256, 4096, 5120])
def test_norm_forward_scatters_to_dense_rows(hip, H, f32):
    """x and rstd on the kept rows of a policy plan (P = [1, 90, 43] at S = 90: shared and unshared rows, an identical pair), y dense:
    every dense row holds vlr_rmsnorm_fwd's row of its source; a y with more rows than the plan stays NaN behind it; and with the twins
    withheld the dropped rows - the rows no kept row maps to - stay NaN"""
    from vlrlhf import prefix_dedup as PD
    plan = PD.build_policy_plan([1, 90, 43], 90)
    M, Mc = plan["M"], plan["Mc"]
    rows, twin, dsrc = (plan[k].int().to(DEV) for k in ("compact_rows", "twin", "dense_src"))
    assert int((twin >= 0).sum()) == M - Mc and int((twin < 0).sum()) > 0
    x = _rnd(Mc, H, seed=H, dtype=torch.float32 if f32 else torch.bfloat16)
    w = (1 + 0.1 * _rnd(H, seed=5).float()).bfloat16()
    entry = "vlr_rmsnorm_fwd_f32" if f32 else "vlr_rmsnorm_fwd"
    yc, rc = nan(Mc, H), nan(Mc, dt=torch.float32)
    hip.call(entry, x, w, yc, rc, Mc, H, 1e-5)
    torch.cuda.synchronize()
    for run in range(2):
        y, r = nan(M + 2, H), nan(Mc + 2, dt=torch.float32)
        hip.call(entry + "_scatter", x, w, y, r, rows, twin, Mc, H, 1e-5)
        torch.cuda.synchronize()
        assert same(y[:M], yc[dsrc.long()]) and same(r[:Mc], rc), run
        assert bool(torch.isnan(y[M:]).all()) and bool(torch.isnan(r[Mc:]).all()), run
    none = torch.full_like(twin, -1)
    y = nan(M, H)
    hip.call(entry + "_scatter", x, w, y, r, rows, none, Mc, H, 1e-5)
    torch.cuda.synchronize()
    kept = torch.zeros(M, dtype=torch.bool, device=DEV)
    kept[rows.long()] = True
    assert same(y[kept], yc) and bool(torch.isnan(y[~kept]).all())
    with pytest.raises(ValueError, match="null argument"):
        hip.call(entry + "_scatter", x, w, y, r, rows, None, Mc, H, 1e-5)


# ------------------------------------------------------------------------------------------------------------ A-row map, forward NT GEMMs
def _a_through_map(hip, M, K, seed):
    """-> (buffer [Msrc + 2][K] with two NaN rows behind it, a_rows [M] that duplicates and reorders, the gathered A [M][K])"""
    Msrc = 3000
    buf = nan(Msrc + 2, K)
    buf[:Msrc] = _rnd(Msrc, K, seed=seed, scale=0.5)
    g = torch.Generator().manual_seed(seed)
    a_rows = torch.randint(0, Msrc, (M,), generator=g).int().to(DEV)
    A = torch.empty(M, K, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gather_rows", buf, a_rows, A, M, K)
    return buf, a_rows, A


def _n256(hip, fn):
    hip.lib_profile_start(1)
    fn()
    n = hip.lib_profile_stop()["gemm256p"][0]
    torch.cuda.synchronize()
    return n


# M = 549: three row tiles, the last partial, one tile per workgroup.  The large M: more output tiles than the 256 workgroups of a persistent
# launch, so some workgroups own two pieces and prefetch the second one's first K tiles through the map.  K = 328: K % 64 != 0, the last K
# tile takes the general staging path; K = 256: the shallowest reduction the kernels take
@pytest.mark.parametrize("K", [256, 328])
@pytest.mark.parametrize("M", [549, 22100])
def test_a_row_map_fused_rope(hip, M, K):
    N, rope_cols, hd, max_pos = 768, 512, 128, 512
    cos = torch.empty(max_pos, hd // 2, dtype=torch.float32, device=DEV)
    sin = torch.empty_like(cos)
    hip.call("vlr_rope_table", cos, sin, max_pos, hd, 10000.0)
    buf, a_rows, A = _a_through_map(hip, M, K, seed=M + K)
    W = _rnd(N, K, seed=3, scale=K ** -0.5)
    pos = (torch.arange(M, device=DEV) % max_pos).int()
    want = nan(M, N)
    n_ref = _n256(hip, lambda: hip.call("vlr_gemm_qkv_rope_bias", A, W, None, want, pos, cos, sin, M, N, rope_cols, K, K, hd, max_pos))
    assert n_ref == 1 and not bool(torch.isnan(want).any())
    for run in range(2):
        out = nan(M + 1, N)
        n = _n256(hip, lambda: hip.call("vlr_gemm_qkv_rope_bias_rows", buf, a_rows, W, None, out, pos, cos, sin, M, N, rope_cols, K, K, hd, max_pos))
        assert n == 1 and same(out[:M], want) and bool(torch.isnan(out[M:]).all()), run
    with pytest.raises(ValueError, match="null row map"):
        hip.call("vlr_gemm_qkv_rope_bias_rows", buf, None, W, None, out, pos, cos, sin, M, N, rope_cols, K, K, hd, max_pos)


@pytest.mark.parametrize("K", [256, 328])
@pytest.mark.parametrize("M", [549, 16700])
def test_a_row_map_fused_swiglu(hip, M, K):
    I = 512
    buf, a_rows, A = _a_through_map(hip, M, K, seed=M + K + 1)
    W = _rnd(2 * I, K, seed=4, scale=K ** -0.5)
    want_gu, want_act = nan(M, 2 * I), nan(M, I)
    assert _n256(hip, lambda: hip.call("vlr_gemm_swiglu", A, W, want_gu, want_act, M, I, K, K, 1)) == 1
    for run in range(2):
        gu, act = nan(M + 1, 2 * I), nan(M + 1, I)
        assert _n256(hip, lambda: hip.call("vlr_gemm_swiglu_rows", buf, a_rows, W, gu, act, M, I, K, K, 1)) == 1
        assert same(gu[:M], want_gu) and same(act[:M], want_act), run
        assert bool(torch.isnan(gu[M:]).all()) and bool(torch.isnan(act[M:]).all()), run
    # store_gu = 0 (the no-grad pass): gate | up is not written
    gu, act = nan(M, 2 * I), nan(M, I)
    hip.call("vlr_gemm_swiglu_rows", buf, a_rows, W, gu, act, M, I, K, K, 0)
    torch.cuda.synchronize()
    assert same(act, want_act) and bool(torch.isnan(gu).all())


# N = 1024 is four column tiles.  M = 12400: 49 x 4 = 196 output tiles, fewer than the workgroups - the per-tile kernel; M = 16700:
# 66 x 4 = 264 - the continuous pipeline on the fp32 stream (a bf16 residual stays on the per-tile kernel).  Both end in a partial row tile
@pytest.mark.parametrize("K", [256, 328])
@pytest.mark.parametrize("M,f32", [(12400, 1), (16700, 1), (16700, 0)], ids=["per-tile-f32", "continuous-f32", "per-tile-bf16"])
def test_a_row_map_residual_projection(hip, M, f32, K):
    N = 1024
    buf, a_rows, A = _a_through_map(hip, M, K, seed=M + K + 2)
    W = _rnd(N, K, seed=5, scale=K ** -0.5)
    dt = torch.float32 if f32 else torch.bfloat16
    res = _rnd(M, N, seed=6, dtype=dt)

    def ref(a, y, r, rows):
        if f32:
            hip.call("vlr_gemm_bf16_f32res", 0, a, W, y, r, rows, N, K, K, K, N, N)
        else:
            hip.call("vlr_gemm_bf16", 0, a, W, y, None, r, rows, N, K, K, K, N, N, 0, 0, 0)
    assert hip.helper("vlr_gemm_peel_rows", M, N) == 0          # the unmapped launch peels nothing at these sizes: one persistent launch
    want = nan(M, N, dt=dt)
    assert _n256(hip, lambda: ref(A, want, res, M)) == 1
    for run in range(2):
        out = nan(M + 1, N, dt=dt)
        assert _n256(hip, lambda: hip.call("vlr_gemm_res_rows", f32, buf, a_rows, W, out, res, M, N, K, 0, 0)) == 1
        assert same(out[:M], want) and bool(torch.isnan(out[M:]).all()), run
    # the caller names the rows of the 128x128 kernel: the last 60 logical rows, one contiguous run of buffer rows, by a plain pointer
    peel, tail0 = 60, 1234
    a2 = a_rows.clone()
    a2[M - peel:] = torch.arange(tail0, tail0 + peel, dtype=torch.int32, device=DEV)
    A2 = torch.empty(M, K, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gather_rows", buf, a2, A2, M, K)
    want = nan(M, N, dt=dt)
    ref(A2, want, res, M - peel)
    ref(A2[M - peel:], want[M - peel:], res[M - peel:], peel)
    out = nan(M + 1, N, dt=dt)
    hip.call("vlr_gemm_res_rows", f32, buf, a2, W, out, res, M, N, K, peel, tail0)
    torch.cuda.synchronize()
    assert same(out[:M], want) and bool(torch.isnan(out[M:]).all())
    # a launch the persistent kernel does not take is an error, not a fallback
    with pytest.raises(ValueError, match="does not take"):
        hip.call("vlr_gemm_res_rows", f32, buf, a_rows, W, out, res, 549, N, K, 0, 0)
