"""Float64 reference and bf16 replay of the CLIP encoder layer's backward (vlr_vit_layer_bwd, csrc/layers.cpp) and of the row-wise
backward kernels of the trainable vision tower (vlr_act_bwd, vlr_vit_embed_ln_bwd, csrc/elementwise.hip), driven through the C ABI by
tests/test_hip_vit_bwd.py.  Plain module, no pytest hooks.

The method is tests/lora_layer_ref.py's: reference(inp) is ONE layer (transformers CLIPEncoderLayer: pre-LN, biased q|k|v / out /
fc1 / fc2, full attention, quick-GELU or erf GELU) written out in float64 torch and differentiated by autograd from a given dy.
replay(inp) is the same layer in float32 with a rounding to bf16 wherever the driver stores bf16, the backward written out call for
call in the order of vlr_vit_layer_bwd (the attention by tests/attn_ref.emulate_kernel_rounding: P and dS rounded to bf16 before their
products).  Two numbers per tensor: err(T) = max|T - ref| / max|ref| and the least-squares scale c(T) = <T, ref> / <ref, ref>.  The
bound of a tensor is 4 x the replay's err and 4 x the replay's |c - 1| + 2^-9 (half a bf16 ulp of 1) - it never comes from the
kernels."""
import math

import torch

from tests import attn_ref as A

F64, F32 = torch.float64, torch.float32
EPS = 1e-5
MARGIN, C_FLOOR = 4.0, 2.0 ** -9
WEIGHTS = ("ln1_w", "ln1_b", "wqkv", "bqkv", "wo", "bo", "ln2_w", "ln2_b", "w1", "b1", "w2", "b2")
HALF_ULP = 2.0 ** -8          # bf16 keeps 8 significant bits: |round_bf16(y) - y| <= half an ulp <= 2^-8 |y|


def bf(t):
    return t.to(torch.bfloat16)


def make(n_img, T, D, heads, mlp, seed=0, act=1):
    """bf16 weights, x [n_img*T][D], two upstream gradients dy / dy2 and old gradient values (for accumulate) of one layer"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)                        # noqa: E731
    M = n_img * T
    w = dict(ln1_w=1 + 0.1 * rn(D), ln1_b=0.1 * rn(D), wqkv=rn(3 * D, D) / math.sqrt(D), bqkv=0.1 * rn(3 * D),
             wo=rn(D, D) / math.sqrt(D), bo=0.1 * rn(D), ln2_w=1 + 0.1 * rn(D), ln2_b=0.1 * rn(D), w1=rn(mlp, D) / math.sqrt(D),
             b1=0.1 * rn(mlp), w2=rn(D, mlp) / math.sqrt(mlp), b2=0.1 * rn(D))
    inp = dict(n_img=n_img, T=T, D=D, heads=heads, mlp=mlp, act=act, M=M, w={k: bf(v) for k, v in w.items()}, x=bf(rn(M, D)),
               dy=bf(rn(M, D)), dy2=bf(rn(M, D)))
    return inp


def act_fn(z, act):
    return z * torch.sigmoid(1.702 * z) if act == 1 else 0.5 * z * (1 + torch.erf(z / math.sqrt(2.0)))


def act_grad(z, act):
    """d act(z) / dz, the formula vlr_act_bwd multiplies dh with"""
    if act == 1:
        s = torch.sigmoid(1.702 * z)
        return s * (1 + 1.702 * z * (1 - s))
    return 0.5 * (1 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


def _ln(x, w, b):
    mu = x.mean(-1, keepdim=True)
    xc = x - mu
    return xc * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + EPS) * w + b


def _layer(inp, x, w, dt):
    n, T, D, nh = inp["n_img"], inp["T"], inp["D"], inp["heads"]
    hd = D // nh
    xn1 = _ln(x, w["ln1_w"], w["ln1_b"])
    qkv = xn1 @ w["wqkv"].t() + w["bqkv"]
    q, k, v = (qkv[:, j * D:(j + 1) * D].reshape(n, T, nh, hd).transpose(1, 2) for j in range(3))
    p = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(hd), -1)
    attn = (p @ v).transpose(1, 2).reshape(n * T, D)
    x_mid = x + attn @ w["wo"].t() + w["bo"]
    xn2 = _ln(x_mid, w["ln2_w"], w["ln2_b"])
    h = act_fn(xn2 @ w["w1"].t() + w["b1"], inp["act"])
    return x_mid + h @ w["w2"].t() + w["b2"]


def reference(inp, dy="dy", device="cpu"):
    """float64 autograd -> {"y": x_out, "dx": dL/dx_in, weight name: its gradient} for L = <x_out, dy>"""
    w = {k: v.to(device, F64).requires_grad_(True) for k, v in inp["w"].items()}
    x = inp["x"].to(device, F64).requires_grad_(True)
    y = _layer(inp, x, w, F64)
    (y * inp[dy].to(device, F64)).sum().backward()
    out = {k: v.grad for k, v in w.items()}
    out["dx"], out["y"] = x.grad, y.detach()
    return out


def _ln_bwd(dy, x, w):
    """(dx, dw, db) of LayerNorm in float32, the formulas of layernorm_bwd_kernel"""
    mu = x.mean(-1, keepdim=True)
    xc = x - mu
    rs = torch.rsqrt((xc * xc).mean(-1, keepdim=True) + EPS)
    xh = xc * rs
    g = dy * w
    dx = rs * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return dx, (dy * xh).sum(0), dy.sum(0)


def replay(inp, dy="dy", device="cpu"):
    """the driver's arithmetic: float32 on bf16 operands, a rounding to bf16 at every store, call for call"""
    r = lambda t: t.to(torch.bfloat16).to(F32)                          # noqa: E731
    n, T, D, nh, act = inp["n_img"], inp["T"], inp["D"], inp["heads"], inp["act"]
    hd = D // nh
    w = {k: v.to(device, F32) for k, v in inp["w"].items()}
    x, d = inp["x"].to(device, F32), inp[dy].to(device, F32)
    heads = lambda t: t.reshape(n, T, nh, hd)                           # noqa: E731
    xn1 = r(_ln(x, w["ln1_w"], w["ln1_b"]))
    qkv = r(xn1 @ w["wqkv"].t() + w["bqkv"])
    q, k, v = (heads(qkv[:, j * D:(j + 1) * D]) for j in range(3))
    attn = A.emulate_kernel_rounding(q, k, v, None, False).o.reshape(n * T, D)
    x_mid = r(x + attn @ w["wo"].t() + w["bo"])
    xn2 = r(_ln(x_mid, w["ln2_w"], w["ln2_b"]))
    z = r(xn2 @ w["w1"].t() + w["b1"])
    h = r(act_fn(z, act))
    out = {"y": r(x_mid + h @ w["w2"].t() + w["b2"])}
    out["w2"], out["b2"] = r(d.t() @ h), r(d.sum(0))
    dz = r(r(d @ w["w2"]) * act_grad(z, act))
    out["w1"], out["b1"] = r(dz.t() @ xn2), r(dz.sum(0))
    dl, dw_, db_ = _ln_bwd(r(dz @ w["w1"]), x_mid, w["ln2_w"])
    d = r(d + dl)                                                        # d x_mid
    out["ln2_w"], out["ln2_b"] = r(dw_), r(db_)
    out["wo"], out["bo"] = r(d.t() @ attn), r(d.sum(0))
    bw = A.emulate_kernel_rounding(q, k, v, None, False, do=heads(r(d @ w["wo"])))
    dqkv = torch.cat([bw.dq.reshape(n * T, D), bw.dk.reshape(n * T, D), bw.dv.reshape(n * T, D)], 1)
    out["wqkv"], out["bqkv"] = r(dqkv.t() @ xn1), r(dqkv.sum(0))
    dl, dw_, db_ = _ln_bwd(r(dqkv @ w["wqkv"]), x, w["ln1_w"])
    out["dx"] = r(d + dl)
    out["ln1_w"], out["ln1_b"] = r(dw_), r(db_)
    return out


TENSORS = WEIGHTS + ("dx", "y")


def err_c(t, ref):
    """-> (err, scale c) of a tensor against the float64 reference"""
    t, ref = t.to(ref.device, F64), ref.to(F64)
    top = float(ref.abs().max())
    if not bool(torch.isfinite(t).all()):
        return float("inf"), float("nan")
    return float((t - ref).abs().max()) / top, float((t * ref).sum() / (ref * ref).sum())


def bounds(err_replay, c_replay):
    return MARGIN * err_replay, MARGIN * abs(c_replay - 1.0) + C_FLOOR


def check(got, ref, rep, names=TENSORS, what=""):
    """asserts every tensor of `got` within the bounds its replay sets; -> {name: (err, bound, |c-1|, bound)}"""
    rows, bad = {}, []
    for nme in names:
        e, c = err_c(got[nme], ref[nme])
        be, bc = bounds(*err_c(rep[nme], ref[nme]))
        rows[nme] = (e, be, abs(c - 1.0), bc)
        if not (e <= be and abs(c - 1.0) <= bc):
            bad.append(nme)
    print(what, " ".join(f"{k}:err={v[0]:.2e}/{v[1]:.2e},c={v[2]:.1e}/{v[3]:.1e}" for k, v in rows.items()))
    assert not bad, f"{what}: outside the replay's bounds: " + ", ".join(f"{k} err {rows[k][0]:.3e} > {rows[k][1]:.3e} or |c-1| {rows[k][2]:.3e} > {rows[k][3]:.3e}" for k in bad)
    return rows


# ---------------------------------------------------------------------------------------------------- embeddings + pre_layrnorm
def embed_make(n_img, T, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)                        # noqa: E731
    names = ("d_cls", "d_pos", "d_w", "d_b")
    shapes = dict(d_cls=(D,), d_pos=(T, D), d_w=(D,), d_b=(D,))
    return dict(n_img=n_img, T=T, D=D, pe=bf(rn(n_img * (T - 1), D)), cls=bf(rn(D)), pos=bf(rn(T, D)), w=bf(1 + 0.1 * rn(D)),
                b=bf(0.1 * rn(D)), dy=bf(rn(n_img * T, D)), old={k: bf(rn(*shapes[k])) for k in names})


def embed_reference(e):
    """float64 autograd of y = LayerNorm(cat(cls, pe) + pos) * w + b for L = <y, dy> -> (y, {d_pe, d_cls, d_pos, d_w, d_b})"""
    n, T, D = e["n_img"], e["T"], e["D"]
    leaf = {k: e[k].to(F64).requires_grad_(True) for k in ("pe", "cls", "pos", "w", "b")}
    v = torch.cat([leaf["cls"].expand(n, 1, D), leaf["pe"].reshape(n, T - 1, D)], 1) + leaf["pos"]
    y = _ln(v, leaf["w"], leaf["b"]).reshape(n * T, D)
    (y * e["dy"].to(F64)).sum().backward()
    return y.detach(), dict(d_pe=leaf["pe"].grad, d_cls=leaf["cls"].grad, d_pos=leaf["pos"].grad, d_w=leaf["w"].grad, d_b=leaf["b"].grad)


def rounding_bound(ref):
    """elementwise bound of a value computed in float32 from exact bf16 inputs and stored as bf16: half a bf16 ulp of the result plus
    float32 noise of the terms it is summed from (the LayerNorm backward cancels terms of the size of the largest result; 2^-16 of it is
    ~250 float32 ulps, generous for sums of <= 64 rows)"""
    return HALF_ULP * ref.abs() * (1 + 2.0 ** -8) + 2.0 ** -16 * ref.abs().max()
