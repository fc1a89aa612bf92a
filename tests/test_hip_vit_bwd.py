"""The backward pieces of a trainable CLIP vision tower at the C ABI: vlr_act_fwd / vlr_act_bwd, vlr_vit_embed_ln_bwd,
vlr_layernorm_bwd_res and vlr_vit_layer_bwd, against the float64 references of tests/vit_layer_ref.py.  Every bound is stated there or
here and comes from the number formats (one bf16 rounding of a float32 result) or from the bf16 replay of the driver - never from the
kernels.  Output buffers start as NaN.  Needs a real MI355X:  pytest -m gpu"""
import ctypes

import pytest
import torch

from tests import vit_layer_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    _hip.ensure_splitk_workspace(DEV, force=True)
    return _hip


def _nan(*shape, dtype=BF):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


# ---------------------------------------------------------------------------------------------------- activation
@pytest.mark.parametrize("act", [1, 2], ids=["quick_gelu", "gelu"])
@pytest.mark.parametrize("n", [1, 7, 8, 1031])
def test_act_fwd_bwd(hip, n, act):
    """n = 1, 7 (tail only), 8 (one vector, no tail), 1031 (vectors, several threads, a 7-element tail); 8 poisoned elements behind the
    n stay untouched.  Bound: one bf16 rounding of the float64 result, plus float32 / __expf noise of act'(z) (|act'| < 1.2) times dh"""
    g = torch.Generator().manual_seed(n)
    z = (3.0 * torch.randn(n, generator=g)).to(BF)
    dh = torch.randn(n, generator=g).to(BF)
    zd, dhd = z.to(DEV), dh.to(DEV)
    h, dz = _nan(n + 8), _nan(n + 8)
    hip.call("vlr_act_fwd", zd, h, n, act)
    hip.call("vlr_act_bwd", zd, dhd, dz, n, act)
    inplace = dhd.clone()
    hip.call("vlr_act_bwd", zd, inplace, inplace, n, act)
    torch.cuda.synchronize()
    assert bool(torch.isnan(h[n:]).all()) and bool(torch.isnan(dz[n:]).all())
    z64, dh64 = z.double(), dh.double()
    ref_h, ref_dz = R.act_fn(z64, act), dh64 * R.act_grad(z64, act)
    eh = (h[:n].cpu().double() - ref_h).abs()
    ed = (dz[:n].cpu().double() - ref_dz).abs()
    print(f"n={n} act={act} max err h {float(eh.max()):.2e} dz {float(ed.max()):.2e}")
    assert bool((eh <= R.HALF_ULP * ref_h.abs() + 1e-5 * z64.abs() + 1e-30).all())
    assert bool((ed <= R.HALF_ULP * ref_dz.abs() + 1e-5 * dh64.abs() + 1e-30).all())
    assert torch.equal(inplace.view(torch.int16), dz[:n].view(torch.int16))


# ---------------------------------------------------------------------------------------------------- embeddings + pre_layrnorm
EMBED_SHAPES = [(n_img, T, D) for n_img in (1, 3) for T in (2, 17) for D in (64, 136)] + [(2, 577, 64)]


@pytest.mark.parametrize("n_img,T,D", EMBED_SHAPES, ids=["x".join(map(str, s)) for s in EMBED_SHAPES])
def test_vit_embed_ln_bwd(hip, n_img, T, D):
    """every output against float64 autograd, accumulate 0 and 1 (on known old values), at R.rounding_bound; the forward it inverts
    is vlr_vit_embed_ln on the same inputs.  T = 577 (CLIP-L's) is past the 256 workgroups of the launch: a workgroup then owns
    positions t, t + 256, t + 512 - three for t < 65, two for the rest - and its d w / d b partials sum over all of them"""
    e = R.embed_make(n_img, T, D, seed=7 * n_img + T + D)
    y_ref, ref = R.embed_reference(e)
    dev = {k: e[k].to(DEV) for k in ("pe", "cls", "pos", "w", "b", "dy")}
    y = _nan(n_img * T, D)
    hip.call("vlr_vit_embed_ln", dev["pe"], dev["cls"], dev["pos"], dev["w"], dev["b"], y, n_img, T, D, R.EPS)
    ws = torch.empty(hip.helper("vlr_layernorm_bwd_workspace_bytes", D), dtype=torch.uint8, device=DEV)
    for accumulate in (0, 1):
        d_pe = _nan(n_img * (T - 1), D)
        outs = {k: (e["old"][k].to(DEV).clone() if accumulate else _nan(*e["old"][k].shape)) for k in e["old"]}
        hip.call("vlr_vit_embed_ln_bwd", dev["dy"], dev["pe"], dev["cls"], dev["pos"], dev["w"], d_pe, outs["d_cls"], outs["d_pos"],
                 outs["d_w"], outs["d_b"], accumulate, ws, n_img, T, D, R.EPS)
        torch.cuda.synchronize()
        got = dict(outs, d_pe=d_pe)
        for k, t in got.items():
            want = ref[k] + (e["old"][k].double() if accumulate and k != "d_pe" else 0.0)
            err = (t.cpu().double() - want).abs()
            tol = R.rounding_bound(want)
            worst = float((err / tol).max())
            print(f"n_img={n_img} T={T} D={D} acc={accumulate} {k}: err/bound {worst:.3f}")
            assert worst <= 1.0, (k, accumulate, worst)
    assert bool(((y.cpu().double() - y_ref).abs() <= R.rounding_bound(y_ref)).all())


def test_layernorm_bwd_res_adds_the_residual_once(hip):
    """vlr_layernorm_bwd_res: dx = dres + LayerNorm-backward with ONE rounding, in place on dres; dw / db are vlr_layernorm_bwd's bits"""
    M, D = 37, 136
    g = torch.Generator().manual_seed(5)
    x, dy, dres = (torch.randn(M, D, generator=g).to(BF) for _ in range(3))
    w = (1 + 0.1 * torch.randn(D, generator=g)).to(BF)
    xd, dyd, wd = x.to(DEV), dy.to(DEV), w.to(DEV)
    ws = torch.empty(hip.helper("vlr_layernorm_bwd_workspace_bytes", D), dtype=torch.uint8, device=DEV)
    dx0, dw0, db0 = _nan(M, D), _nan(D), _nan(D)
    hip.call("vlr_layernorm_bwd", dyd, xd, wd, R.EPS, dx0, dw0, db0, 0, ws, M, D)
    dx1, dw1, db1 = dres.to(DEV).clone(), _nan(D), _nan(D)
    hip.call("vlr_layernorm_bwd_res", dyd, xd, wd, R.EPS, dx1, dx1, dw1, db1, 0, ws, M, D)
    torch.cuda.synchronize()
    assert torch.equal(dw0.view(torch.int16), dw1.view(torch.int16)) and torch.equal(db0.view(torch.int16), db1.view(torch.int16))
    ln, _, _ = R._ln_bwd(dy.double(), x.double(), w.double())
    want = dres.double() + ln
    assert bool(((dx1.cpu().double() - want).abs() <= R.rounding_bound(want)).all())


# ---------------------------------------------------------------------------------------------------- the encoder layer
SHAPES = [(2, 17, 64, 1, 128), (3, 65, 128, 2, 256), (1, 577, 1024, 16, 4096)]      # (n_img, T, D, heads, mlp); the last is CLIP-L


class Layer:
    """device buffers and ctypes structs of one vlr_vit_layer_fwd / _bwd call"""

    def __init__(self, hip, inp):
        self.hip, self.inp = hip, inp
        n, T, D, nh, F = inp["n_img"], inp["T"], inp["D"], inp["heads"], inp["mlp"]
        M, Sp = n * T, (T + 63) // 64 * 64
        self.cfg = hip.VitCfg(D, F, nh, D // nh, R.EPS, inp["act"], 0, 0.0)
        self.w = {k: v.to(DEV) for k, v in inp["w"].items()}
        self.wstruct = hip.VitLayerWeights(*[self.w[k].data_ptr() for k in R.WEIGHTS])
        self.x = inp["x"].to(DEV)
        self.fws_t = dict(xn=_nan(M, D), qkv=_nan(M, 3 * D), attn=_nan(M, D), h=_nan(M, F))
        self.fws = hip.VitWs(*[self.fws_t[k].data_ptr() for k in ("xn", "qkv", "attn", "h")])
        nb = hip.helper("vlr_vit_layer_bwd_workspace_bytes", D, F)
        t = dict(xn1=_nan(M, D), qkv=_nan(M, 3 * D), attn=_nan(M, D), lse=_nan(n, nh, Sp, dtype=torch.float32), x_mid=_nan(M, D),
                 xn2=_nan(M, D), z=_nan(M, F), h=_nan(M, F), dh=_nan(M, F), dxn=_nan(M, D), dattn=None, dqkv=_nan(M, 3 * D),
                 delta=_nan(n, nh, Sp, dtype=torch.float32), norm_ws=torch.empty(nb, dtype=torch.uint8, device=DEV))
        t["dattn"] = t["dxn"]                      # the two may share a buffer (include/vlr.h)
        self.bws_t = t
        self.bws = hip.VitBwdWs(*[t[k].data_ptr() for k, _ in hip.VitBwdWs._fields_])

    def forward(self):
        y = self.x.clone()
        self.hip.call("vlr_vit_layer_fwd", self.cfg, self.wstruct, self.fws, y, self.inp["n_img"], self.inp["T"])
        return y

    def backward(self, dy, grads, accumulate):
        """grads {name: tensor} are written (or accumulated into); -> dx"""
        gs = self.hip.VitLayerGrads(*[grads[k].data_ptr() for k in R.WEIGHTS])
        dx = dy.to(DEV).clone()
        self.hip.call("vlr_vit_layer_bwd", self.cfg, self.wstruct, gs, accumulate, self.x, self.bws, dx, self.inp["n_img"], self.inp["T"])
        return dx

    def nan_grads(self):
        return {k: _nan(*v.shape) for k, v in self.w.items()}


@pytest.fixture(scope="module", params=SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def layer_case(request, hip):
    """one layer per shape, its float64 reference and bf16 replay (computed once, on the device), shared by the tests below"""
    inp = R.make(*request.param, seed=sum(request.param))
    return Layer(hip, inp), R.reference(inp, device=DEV), R.replay(inp, device=DEV)


def test_vit_layer_bwd_every_gradient(layer_case):
    L, ref, rep = layer_case
    y0 = L.forward()
    x_before = L.x.clone()
    grads = L.nan_grads()
    got = dict(grads, dx=L.backward(L.inp["dy"], grads, 0))
    y1 = L.forward()
    torch.cuda.synchronize()
    got["y"] = y1
    R.check(got, ref, rep, what="x".join(str(L.inp[k]) for k in ("n_img", "T", "D", "heads", "mlp")))
    # the forward is the forward: its output does not depend on a backward having run, and the backward leaves x_in alone
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16)) and torch.equal(x_before.view(torch.int16), L.x.view(torch.int16))
    # fixed summation orders: a second call gives the same bits
    grads2 = L.nan_grads()
    dx2 = L.backward(L.inp["dy"], grads2, 0)
    torch.cuda.synchronize()
    assert torch.equal(dx2.view(torch.int16), got["dx"].view(torch.int16))
    for k in R.WEIGHTS:
        assert torch.equal(grads[k].view(torch.int16), grads2[k].view(torch.int16)), k


def test_vit_layer_bwd_accumulate(layer_case):
    """accumulate = 1 on top of the gradients of dy equals the two accumulate = 0 results summed, within one bf16 rounding of each:
    |g - (g1 + g2)| <= 2^-8 |g2| + 2^-8 |g1 + g2| <= 2^-7 (|g1| + |g2|) (bf16's unit roundoff is 2^-8), plus float32 noise of the sum
    order (2^-16 of the largest)"""
    L, _, _ = layer_case
    g1, g2 = L.nan_grads(), L.nan_grads()
    L.backward(L.inp["dy"], g1, 0)
    dx2 = L.backward(L.inp["dy2"], g2, 0)
    acc = {k: v.clone() for k, v in g1.items()}
    dx_acc = L.backward(L.inp["dy2"], acc, 1)
    torch.cuda.synchronize()
    assert torch.equal(dx_acc.view(torch.int16), dx2.view(torch.int16))      # dx never accumulates
    for k in R.WEIGHTS:
        a, b, c = g1[k].double(), g2[k].double(), acc[k].double()
        tol = 2 * R.HALF_ULP * (a.abs() + b.abs()) + 2.0 ** -16 * (a + b).abs().max()
        worst = float(((c - (a + b)).abs() / tol).max())
        assert worst <= 1.0, (k, worst)


def test_vit_layer_bwd_refuses_a_padded_head_dim(hip):
    inp = R.make(1, 17, 64, 1, 128)
    L = Layer(hip, inp)
    L.cfg.head_dim_pad = 128
    with pytest.raises(ValueError, match="padded head_dim"):
        L.backward(inp["dy"], L.nan_grads(), 0)
    assert ctypes.sizeof(hip.VitBwdWs) == 14 * ctypes.sizeof(ctypes.c_void_p)
