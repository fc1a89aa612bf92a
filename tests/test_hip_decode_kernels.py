"""The KV-cache decoding kernels (csrc/decode.hip) through the C ABI on the MI355X, against fp32 torch and against the prefill kernels
they stand in for: the skinny GEMM and its five epilogues, the cache write, split-KV decode attention and the composed decode layer.
Outputs are NaN-poisoned before every call.  Needs a real MI355X:  pytest -m gpu"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return _hip


def rnd(*shape, scale=1.0, seed=0, dtype=torch.bfloat16):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def relerr(a, b):
    a, b = a.float(), b.float()
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-12)


def check(a, b, tol, what=""):
    e = relerr(a, b)
    assert math.isfinite(e) and e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"


def nan_like(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def gemv(hip, mode, X, W, Y, M, N, K, bias=None, res=None, ldr=0, pos=None, cos=None, sin=None, rope_cols=0, hd=128, max_pos=0):
    ws = torch.empty(int(hip.lib().vlr_gemv_workspace_bytes(M, N, K)), dtype=torch.uint8, device=DEV)
    hip.call("vlr_gemv_bf16", mode, X, X.shape[1], W, Y, Y.shape[1], bias, res, ldr, pos, cos, sin, rope_cols, hd, max_pos, M, N, K, ws)


# ---------------------------------------------------------------------------------------------------- skinny GEMM
SHAPES_7B = [(4096, 12288), (4096, 4096), (4096, 22016), (11008, 4096), (4096, 32000)]      # (K, N): qkv, o, gate|up, down, lm-head
SHAPES_MISTRAL = [(4096, 6144), (4096, 28672), (14336, 4096)]
SHAPES_FIXTURE = [(128, 192), (128, 128), (256, 192), (136, 200)]


@pytest.mark.parametrize("K,N", SHAPES_7B + SHAPES_MISTRAL + SHAPES_FIXTURE)
@pytest.mark.parametrize("M", [1, 3, 8, 16])
def test_gemv_plain(hip, M, K, N):
    """Y = X W^T at bf16 and fp32 out against fp32 torch; the fp32 result is bit-identical run to run"""
    X, W = rnd(M, K, seed=1), rnd(N, K, scale=0.05, seed=2)
    ref = X.float() @ W.float().T
    Y = nan_like((M, N), torch.bfloat16)
    gemv(hip, hip.GEMV_BF16, X, W, Y, M, N, K)
    F = nan_like((M, N), torch.float32)
    gemv(hip, hip.GEMV_F32, X, W, F, M, N, K)
    F2 = nan_like((M, N), torch.float32)
    gemv(hip, hip.GEMV_F32, X, W, F2, M, N, K)
    torch.cuda.synchronize()
    check(Y, ref, 8e-3, "bf16 out")
    check(F, ref, 1e-4, "fp32 out")
    assert torch.equal(F, F2)


@pytest.mark.parametrize("M", [3, 16])
def test_gemv_bias_residual_epilogues(hip, M):
    K, N = 4096, 4096
    X, W = rnd(M, K, seed=3), rnd(N, K, scale=0.05, seed=4)
    bias, res = rnd(N, seed=5), rnd(M, N, seed=6)
    acc = X.float() @ W.float().T
    Y = nan_like((M, N), torch.bfloat16)
    gemv(hip, hip.GEMV_BF16, X, W, Y, M, N, K, bias=bias, res=res, ldr=N)
    # fp32 residual stream, in place (o_proj / down_proj of vlr_llama_cfg.resid_f32)
    R = torch.randn(M, N, generator=torch.Generator().manual_seed(7)).to(DEV)
    R0 = R.clone()
    gemv(hip, hip.GEMV_F32RES, X, W, R, M, N, K, res=R, ldr=N)
    # bf16 residual in place
    Rb = res.clone()
    gemv(hip, hip.GEMV_BF16, X, W, Rb, M, N, K, res=Rb, ldr=N)
    torch.cuda.synchronize()
    check(Y, acc + bias.float() + res.float(), 8e-3, "bias + residual")
    check(R, acc + R0, 1e-5, "fp32 residual in place")
    check(Rb, acc + res.float(), 8e-3, "bf16 residual in place")


@pytest.mark.parametrize("M,H,nh,nkv,bias", [(4, 4096, 32, 32, False), (3, 4096, 32, 8, True), (16, 4096, 32, 8, False),
                                             (2, 128, 1, 1, True), (5, 256, 2, 1, False)])
def test_gemv_qkv_rope_matches_prefill_kernel(hip, M, H, nh, nkv, bias):
    """q|k|v + bias + rotate-half RoPE at per-row positions: against fp32 torch and against vlr_gemm_qkv_rope_bias on the same rows
    (within bf16 rounding)"""
    hd, max_pos = 128, 4096
    N, rc = (nh + 2 * nkv) * hd, (nh + nkv) * hd
    cos = torch.empty(max_pos, hd // 2, dtype=torch.float32, device=DEV)
    sin = torch.empty_like(cos)
    hip.call("vlr_rope_table", cos, sin, max_pos, hd, 10000.0)
    X, W = rnd(M, H, seed=8), rnd(N, H, scale=0.05, seed=9)
    b = rnd(N, seed=10) if bias else None
    pos = torch.tensor([(37 * i + 5) % 3000 for i in range(M)], dtype=torch.int32, device=DEV)
    Y = nan_like((M, N), torch.bfloat16)
    gemv(hip, hip.GEMV_QKV_ROPE, X, W, Y, M, N, H, bias=b, pos=pos, cos=cos, sin=sin, rope_cols=rc, hd=hd, max_pos=max_pos)
    P = nan_like((M, N), torch.bfloat16)
    hip.call("vlr_gemm_qkv_rope_bias", X, W, b, P, pos, cos, sin, M, N, rc, H, H, hd, max_pos)
    torch.cuda.synchronize()
    acc = X.float() @ W.float().T + (b.float() if bias else 0.0)
    ref = acc.clone()
    heads = acc[:, :rc].reshape(M, -1, hd)
    x1, x2 = heads[..., :hd // 2], heads[..., hd // 2:]
    c, s = cos[pos.long()][:, None], sin[pos.long()][:, None]
    ref[:, :rc] = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).reshape(M, rc)
    check(Y, ref, 8e-3, "rope vs fp32")
    check(Y, P.float(), 1.6e-2, "rope vs vlr_gemm_qkv_rope_bias")


@pytest.mark.parametrize("M,H,I", [(1, 4096, 11008), (4, 4096, 11008), (16, 4096, 14336), (3, 128, 256)])
def test_gemv_swiglu(hip, M, H, I):
    X, W = rnd(M, H, seed=11), rnd(2 * I, H, scale=0.05, seed=12)
    A = nan_like((M, I), torch.bfloat16)
    gemv(hip, hip.GEMV_SWIGLU, X, W, A, M, 2 * I, H)
    torch.cuda.synchronize()
    gu = X.float() @ W.float().T
    g, u = gu[:, :I], gu[:, I:]
    check(A, torch.nn.functional.silu(g) * u, 1e-2, "swiglu")


# ---------------------------------------------------------------------------------------------------- cache write
@pytest.mark.parametrize("B,S,nkv,slot0,cap", [(2, 37, 1, 0, 64), (4, 1, 32, 1599, 1727), (3, 200, 8, 5, 300)])
def test_kv_cache_write_exact(hip, B, S, nkv, slot0, cap):
    hd, nh = 128, 2 * nkv
    Nq, Nkv = nh * hd, nkv * hd
    N = Nq + 2 * Nkv
    qkv = rnd(B * S, N, seed=13)
    kc = torch.full((B, nkv, cap, hd), float("nan"), dtype=torch.bfloat16, device=DEV)
    vc = kc.clone()
    hip.call("vlr_kv_cache_write", qkv[:, Nq:], qkv[:, Nq + Nkv:], N, kc, vc, B, S, nkv, hd, cap, slot0)
    torch.cuda.synchronize()
    k = qkv[:, Nq:Nq + Nkv].reshape(B, S, nkv, hd).transpose(1, 2)
    v = qkv[:, Nq + Nkv:].reshape(B, S, nkv, hd).transpose(1, 2)
    assert torch.equal(kc[:, :, slot0:slot0 + S].view(torch.int16), k.contiguous().view(torch.int16))
    assert torch.equal(vc[:, :, slot0:slot0 + S].view(torch.int16), v.contiguous().view(torch.int16))
    assert bool(torch.isnan(kc[:, :, :slot0].float()).all()) and bool(torch.isnan(kc[:, :, slot0 + S:].float()).all())


# ---------------------------------------------------------------------------------------------------- decode attention
@pytest.mark.parametrize("nh,nkv", [(32, 32), (32, 8), (1, 1), (2, 1)])
@pytest.mark.parametrize("B,L", [(1, 1), (4, 63), (8, 64), (4, 1599), (1, 4975)])
def test_attn_decode_matches_last_row_of_prefill(hip, nh, nkv, B, L):
    """vlr_attn_decode_gqa over a cache filled from q|k|v rows == the last row of vlr_attn_fwd_gqa (causal) on the same rows, under
    left-padded key masks; two calls are bit-identical"""
    hd = 128
    Hq, Hkv = nh * hd, nkv * hd
    N = Hq + 2 * Hkv
    qkv = rnd(B * L, N, seed=14)
    km = torch.ones(B, L, dtype=torch.int32, device=DEV)
    for b in range(1, B):                                    # left padding of every row but the first
        km[b, :min(L - 1, 7 * b)] = 0
    scale = 1.0 / math.sqrt(hd)
    Sp = (L + 63) // 64 * 64
    o = nan_like((B * L, Hq), torch.bfloat16)
    lse = torch.zeros(B, nh, Sp, dtype=torch.float32, device=DEV)
    hip.call("vlr_attn_fwd_gqa", qkv, qkv[:, Hq:], qkv[:, Hq + Hkv:], N, o, Hq, lse, km, B, L, nh, nkv, hd, 1, scale)
    cap = L + 9
    kc = torch.full((B, nkv, cap, hd), float("nan"), dtype=torch.bfloat16, device=DEV)
    vc = kc.clone()
    hip.call("vlr_kv_cache_write", qkv[:, Hq:], qkv[:, Hq + Hkv:], N, kc, vc, B, L, nkv, hd, cap, 0)
    kmc = torch.zeros(B, cap, dtype=torch.int32, device=DEV)
    kmc[:, :L] = km
    q = qkv.view(B, L, N)[:, L - 1].contiguous()
    ws = torch.empty(int(hip.lib().vlr_attn_decode_workspace_bytes(B, nh, cap)), dtype=torch.uint8, device=DEV)
    od = nan_like((B, Hq), torch.bfloat16)
    hip.call("vlr_attn_decode_gqa", q, N, kc, vc, kmc, od, Hq, ws, B, nh, nkv, hd, cap, L, scale)
    od2 = nan_like((B, Hq), torch.bfloat16)
    hip.call("vlr_attn_decode_gqa", q, N, kc, vc, kmc, od2, Hq, ws, B, nh, nkv, hd, cap, L, scale)
    torch.cuda.synchronize()
    last = o.view(B, L, Hq)[:, L - 1]
    # fp32 eager reference of the last row
    x = qkv.float().view(B, L, N)
    qf = x[:, L - 1, :Hq].reshape(B, nh, 1, hd)
    kf = x[:, :, Hq:Hq + Hkv].reshape(B, L, nkv, hd).transpose(1, 2).repeat_interleave(nh // nkv, dim=1)
    vf = x[:, :, Hq + Hkv:].reshape(B, L, nkv, hd).transpose(1, 2).repeat_interleave(nh // nkv, dim=1)
    s = (qf @ kf.transpose(-1, -2)) * scale
    s = s.masked_fill(km[:, None, None, :] == 0, float("-inf"))
    ref = (s.softmax(-1) @ vf).reshape(B, Hq)
    check(od, ref, 1.2e-2, "decode vs fp32")
    check(od, last.float(), 1.6e-2, "decode vs last row of vlr_attn_fwd_gqa")
    assert torch.equal(od.view(torch.int16), od2.view(torch.int16))


# ---------------------------------------------------------------------------------------------------- composed decode layer
def _acts(hip, B, S, H, I, nh, Nq, Nqkv, rdt):
    M = B * S
    Sp = (S + 63) // 64 * 64
    t = dict(xn1=torch.empty(M, H, dtype=torch.bfloat16, device=DEV), rstd1=torch.empty(M, device=DEV),
             qkv=torch.empty(M, Nqkv, dtype=torch.bfloat16, device=DEV), attn=torch.empty(M, Nq, dtype=torch.bfloat16, device=DEV),
             lse=torch.empty(B, nh, Sp, device=DEV), x_mid=torch.empty(M, H, dtype=rdt, device=DEV),
             xn2=torch.empty(M, H, dtype=torch.bfloat16, device=DEV), rstd2=torch.empty(M, device=DEV),
             gu=torch.empty(M, 2 * I, dtype=torch.bfloat16, device=DEV), act=torch.empty(M, I, dtype=torch.bfloat16, device=DEV),
             x_out=torch.empty(M, H, dtype=rdt, device=DEV))
    t["struct"] = hip.LayerActs(*(t[n].data_ptr() for n in ("xn1", "rstd1", "qkv", "attn", "lse", "x_mid", "xn2", "rstd2", "gu", "act", "x_out")))
    return t


@pytest.mark.parametrize("resid_f32", [1, 0])
@pytest.mark.parametrize("H,I,nh,nkv,B,S", [(4096, 11008, 32, 32, 2, 190), (4096, 14336, 32, 8, 3, 130), (256, 256, 2, 1, 2, 40)])
def test_decoder_layer_decode_matches_prefill(hip, resid_f32, H, I, nh, nkv, B, S):
    """prefill S rows (vlr_decoder_layer_fwd_ex + cache write), then decode row S + 1 (vlr_decoder_layer_decode) == the last row of
    vlr_decoder_layer_fwd_ex on S + 1 rows, at true widths, both residual streams"""
    hd, max_pos = 128, 4096
    Nq, Nkv = nh * hd, nkv * hd
    N = Nq + 2 * Nkv
    cos = torch.empty(max_pos, hd // 2, dtype=torch.float32, device=DEV)
    sin = torch.empty_like(cos)
    hip.call("vlr_rope_table", cos, sin, max_pos, hd, 10000.0)
    cfg = hip.LlamaCfg(H, I, nh, hd, 1e-5, max_pos, cos.data_ptr(), sin.data_ptr(), nkv, resid_f32)
    sc = 1.0 / math.sqrt(H)
    W = dict(ln1=(1 + 0.1 * rnd(H, seed=20).float()).bfloat16(), wqkv=rnd(N, H, scale=sc, seed=21), wo=rnd(H, Nq, scale=sc, seed=22),
             ln2=(1 + 0.1 * rnd(H, seed=23).float()).bfloat16(), wgu=rnd(2 * I, H, scale=sc, seed=24), wdown=rnd(H, I, scale=1 / math.sqrt(I), seed=25))
    lw = hip.LayerWeights(*(W[k].data_ptr() for k in ("ln1", "wqkv", "wo", "ln2", "wgu", "wdown")), None)
    rdt = torch.float32 if resid_f32 else torch.bfloat16
    S1 = S + 1
    x = rnd(B, S1, H, seed=26, dtype=torch.float32).to(rdt)
    km = torch.ones(B, S1, dtype=torch.int32, device=DEV)
    for b in range(1, B):
        km[b, :5 * b] = 0                                    # left padding
    pos = (km.cumsum(1) - 1).to(torch.int32)
    pos[km == 0] = 1
    # full pass over S + 1 rows
    af = _acts(hip, B, S1, H, I, nh, Nq, N, rdt)
    hip.call("vlr_decoder_layer_fwd_ex", cfg, lw, af["struct"], x.reshape(B * S1, H), pos, km, B, S1, 0)
    # prefill over S rows + cache write
    xp = x[:, :S].contiguous()
    ap = _acts(hip, B, S, H, I, nh, Nq, N, rdt)
    hip.call("vlr_decoder_layer_fwd_ex", cfg, lw, ap["struct"], xp.reshape(B * S, H), pos[:, :S].contiguous(), km[:, :S].contiguous(), B, S, 0)
    cap = S1 + 3
    kc = torch.full((B, nkv, cap, hd), float("nan"), dtype=torch.bfloat16, device=DEV)
    vc = kc.clone()
    hip.call("vlr_kv_cache_write", ap["qkv"][:, Nq:], ap["qkv"][:, Nq + Nkv:], N, kc, vc, B, S, nkv, hd, cap, 0)
    kmc = torch.zeros(B, cap, dtype=torch.int32, device=DEV)
    kmc[:, :S1] = km
    mb = min(B, 16)
    gb = max(int(hip.lib().vlr_gemv_workspace_bytes(mb, n, k)) for n, k in ((N, H), (H, Nq), (2 * I, H), (H, I)))
    ab = int(hip.lib().vlr_attn_decode_workspace_bytes(B, nh, cap))
    d = dict(xn=torch.empty(B, H, dtype=torch.bfloat16, device=DEV), rstd=torch.empty(B, device=DEV),
             qkv=torch.empty(B, N, dtype=torch.bfloat16, device=DEV), attn=torch.empty(B, Nq, dtype=torch.bfloat16, device=DEV),
             act=torch.empty(B, I, dtype=torch.bfloat16, device=DEV), gemv=torch.empty(gb, dtype=torch.uint8, device=DEV),
             attn_ws=torch.empty(ab, dtype=torch.uint8, device=DEV))
    dws = hip.DecodeWs(d["xn"].data_ptr(), d["rstd"].data_ptr(), d["qkv"].data_ptr(), d["attn"].data_ptr(), d["act"].data_ptr(),
                       d["gemv"].data_ptr(), gb, d["attn_ws"].data_ptr(), ab)
    xd = x[:, S].contiguous()
    x_in = xd.clone()
    pd = pos[:, S].contiguous()
    hip.call("vlr_decoder_layer_decode", cfg, lw, dws, xd, pd, kc, vc, kmc, B, cap, S)
    torch.cuda.synchronize()
    full = af["x_out"].view(B, S1, H)[:, S]
    # the layer's update (the residual dominates x_out): the decode pass against the prefill pass, within bf16 rounding
    check(xd.float() - x_in.float(), full.float() - x_in.float(), 2e-2, "decode layer update")
    assert torch.isfinite(xd.float()).all()
    # the cache column of the new token holds its K / V row as the full pass computed it (within bf16 rounding)
    kfull = af["qkv"].view(B, S1, N)[:, S, Nq:Nq + Nkv].reshape(B, nkv, hd)
    check(kc[:, :, S], kfull, 1.6e-2, "new K column")
    # the workspaces are validated against the capacity
    bad = hip.DecodeWs(d["xn"].data_ptr(), d["rstd"].data_ptr(), d["qkv"].data_ptr(), d["attn"].data_ptr(), d["act"].data_ptr(),
                       d["gemv"].data_ptr(), gb, d["attn_ws"].data_ptr(), ab - 4)
    with pytest.raises(ValueError, match="attn_ws"):
        hip.call("vlr_decoder_layer_decode", cfg, lw, bad, xd, pd, kc, vc, kmc, B, cap, S)
