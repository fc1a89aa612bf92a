"""Kernel-level parity: every vlr_* entry point (called through the C ABI) against a plain PyTorch fp32 reference of
the same op / the CPU oracle, on seeded inputs.  Needs a real MI355X:  pytest -m gpu"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import llava_dpo_oracle as O  # noqa: E402  (checker only)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return _hip


DEV = "cuda"


def rnd(*shape, scale=1.0, seed=0, dtype=torch.bfloat16):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def relerr(a, b):
    a, b = a.float(), b.float()
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-12)


def check(a, b, tol, what=""):
    e = relerr(a, b)
    assert math.isfinite(e) and e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"


# ---------------------------------------------------------------------------------------------------- GEMM
GEMM_SHAPES = [(256, 256, 128), (128, 128, 64), (200, 136, 72), (1000, 512, 320), (96, 1032, 256), (2048, 4096, 1024),
               # >= 192 tiles of 256x256: the LDS-DMA 256-tile kernel (ragged M/N edges, K = one / odd number of tiles)
               (4096, 3072, 256), (4000, 3336, 192), (3592, 4104, 64), (12792, 4096, 320),
               # K tail of the k-contiguous operands (K % 64 = 8): the last K tile takes the zero-filling DMA path
               (4096, 3072, 328)]


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("shape", GEMM_SHAPES)
def test_gemm_layouts(hip, layout, shape):
    M, N, K = shape
    if layout == 2 and (M % 4 or N % 4):
        pytest.skip("alignment")
    if layout == 2 and M * N >= 192 * 65536:
        K = K + 40            # wgrad contracts over the token count: not a multiple of 64 -> zero-filled K tail
    a = rnd(M, K, seed=1)
    b = rnd(N, K, seed=2)
    ref = a.float() @ b.float().t()
    A = a if layout != 2 else a.t().contiguous()           # TN: A stored [K][M]
    Bm = b if layout == 0 else b.t().contiguous()          # NN/TN: B stored [K][N]
    lda = K if layout != 2 else M
    ldb = K if layout == 0 else N
    c = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_bf16", layout, A, Bm, c, None, None, M, N, K, lda, ldb, N, 0, 0, 0, 0)
    torch.cuda.synchronize()
    check(c, ref, 8e-3, f"gemm layout {layout} {shape}")


def test_gemm_asymmetric_identity(hip):
    """A = I with an asymmetric B catches row/col swaps in the C write (guide rule 16)."""
    n = 128
    a = torch.eye(n, dtype=torch.bfloat16, device=DEV)
    b = (torch.arange(n * n, device=DEV).reshape(n, n) % 251).to(torch.bfloat16)
    c = torch.empty(n, n, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_bf16", 0, a, b, c, None, None, n, n, n, n, n, n, 0, 0, 0, 0)
    torch.cuda.synchronize()
    assert torch.equal(c.float(), b.float().t())


def test_gemm_epilogues(hip):
    M, N, K = 300, 264, 136
    a, b = rnd(M, K, seed=3, scale=0.3), rnd(N, K, seed=4, scale=0.3)
    bias, res = rnd(N, seed=5), rnd(M, N, seed=6)
    base = a.float() @ b.float().t()
    for act, fn in ((0, lambda x: x), (1, lambda x: x * torch.sigmoid(1.702 * x)), (2, lambda x: F.gelu(x))):
        c = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        hip.call("vlr_gemm_bf16", 0, a, b, c, bias, res, M, N, K, K, K, N, N, act, 0, 0)
        torch.cuda.synchronize()
        check(c, fn(base + bias.float()) + res.float(), 8e-3, f"epilogue act {act}")
    # accumulate into bf16 C, and fp32 output with accumulate
    c = rnd(M, N, seed=7)
    c0 = c.clone()
    hip.call("vlr_gemm_bf16", 0, a, b, c, None, None, M, N, K, K, K, N, 0, 0, 1, 0)
    torch.cuda.synchronize()
    check(c, base + c0.float(), 8e-3, "accumulate bf16")
    cf = torch.ones(M, N, dtype=torch.float32, device=DEV)
    hip.call("vlr_gemm_bf16", 0, a, b, cf, bias, None, M, N, K, K, K, N, 0, 0, 1, 1)
    torch.cuda.synchronize()
    check(cf, base + bias.float() + 1.0, 1e-4, "fp32 out")
    # strided C (column block of a wider buffer) - how q|k|v and gate|up are produced
    wide = torch.zeros(M, 2 * N, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_bf16", 0, a, b, wide[:, N:], None, None, M, N, K, K, K, 2 * N, 0, 0, 0, 0)
    torch.cuda.synchronize()
    check(wide[:, N:], base, 8e-3, "strided C")
    assert float(wide[:, :N].abs().max()) == 0.0


def test_gemm_bad_args(hip):
    a = rnd(8, 8)
    with pytest.raises(ValueError):
        hip.call("vlr_gemm_bf16", 7, a, a, a, None, None, 8, 8, 8, 8, 8, 8, 0, 0, 0, 0)
    with pytest.raises(ValueError):
        hip.call("vlr_gemm_bf16", 0, a, a, a, None, None, 8, 8, 7, 8, 8, 8, 0, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ norms etc.
@pytest.mark.parametrize("M,H", [(37, 256), (513, 4096), (64, 1024)])
def test_rmsnorm_fwd_bwd(hip, M, H):
    x, w, dy, dres = rnd(M, H, seed=1), (1 + 0.1 * rnd(H, seed=2).float()).bfloat16(), rnd(M, H, seed=3), rnd(M, H, seed=4)
    y = torch.empty_like(x)
    rstd = torch.empty(M, dtype=torch.float32, device=DEV)
    hip.call("vlr_rmsnorm_fwd", x, w, y, rstd, M, H, 1e-5)
    xf = x.float().requires_grad_(True)
    wf = w.float().requires_grad_(True)
    ref = O.rms_norm(xf, wf, 1e-5)
    torch.cuda.synchronize()
    check(y, ref, 6e-3, "rmsnorm fwd")
    check(rstd, torch.rsqrt(x.float().pow(2).mean(-1) + 1e-5), 1e-5, "rstd")
    (ref * dy.float()).sum().backward()
    ws = torch.empty(hip.helper("vlr_rmsnorm_bwd_workspace_bytes", H), dtype=torch.uint8, device=DEV)
    dx = torch.empty_like(x)
    dw = rnd(H, seed=9)
    dw0 = dw.clone()
    hip.call("vlr_rmsnorm_bwd", dy, x, w, rstd, dres, dx, dw, 1, ws, M, H)
    torch.cuda.synchronize()
    check(dx, xf.grad + dres.float(), 8e-3, "rmsnorm dx")
    check(dw, wf.grad + dw0.float(), 8e-3, "rmsnorm dw (accumulate)")
    hip.call("vlr_rmsnorm_bwd", dy, x, w, rstd, None, dx, dw, 0, ws, M, H)
    torch.cuda.synchronize()
    check(dx, xf.grad, 8e-3, "rmsnorm dx no residual")
    check(dw, wf.grad, 8e-3, "rmsnorm dw")


def test_layernorm_and_vit_embed(hip):
    M, D = 77, 1024
    x, w, b = rnd(M, D, seed=1), rnd(D, seed=2), rnd(D, seed=3)
    y = torch.empty_like(x)
    hip.call("vlr_layernorm_fwd", x, w, b, y, M, D, 1e-5)
    torch.cuda.synchronize()
    check(y, F.layer_norm(x.float(), (D,), w.float(), b.float(), 1e-5), 8e-3, "layernorm")
    n, T = 3, 17
    pe, cls, pos = rnd(n * (T - 1), D, seed=4), rnd(D, seed=5), rnd(T, D, seed=6)
    out = torch.empty(n * T, D, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_vit_embed_ln", pe, cls, pos, w, b, out, n, T, D, 1e-5)
    torch.cuda.synchronize()
    emb = torch.cat([cls.float().expand(n, 1, D), pe.float().reshape(n, T - 1, D)], 1) + pos.float()[None]
    check(out, F.layer_norm(emb, (D,), w.float(), b.float(), 1e-5).reshape(n * T, D), 8e-3, "vit embed+ln")


def test_im2col(hip):
    n, S, Pp = 2, 56, 14
    Kp = 592
    px = torch.randn(n, 3, S, S, device=DEV)
    out = torch.empty(n * 16, Kp, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_im2col", px, out, n, S, Pp, Kp)
    torch.cuda.synchronize()
    g = S // Pp
    ref = px.reshape(n, 3, g, Pp, g, Pp).permute(0, 2, 4, 1, 3, 5).reshape(n * g * g, 3 * Pp * Pp)
    assert torch.equal(out[:, :588], ref.bfloat16())
    assert float(out[:, 588:].abs().max()) == 0.0


def test_rope(hip):
    B, S, nh, hd = 2, 50, 3, 128
    H = nh * hd
    qkv = rnd(B * S, 3 * H, seed=1)
    pos = torch.randint(0, 300, (B, S), device=DEV, dtype=torch.int32)
    cos_t = torch.empty(512, hd // 2, dtype=torch.float32, device=DEV)
    sin_t = torch.empty_like(cos_t)
    hip.call("vlr_rope_table", cos_t, sin_t, 512, hd, 10000.0)
    cos, sin = O.rope_tables(pos.cpu().long(), hd)
    torch.cuda.synchronize()
    check(cos_t[pos.long()], cos[..., : hd // 2].to(DEV), 2e-4, "cos table")
    x = qkv.clone()
    hip.call("vlr_rope", x, pos, cos_t, sin_t, B * S, H, hd, 3 * H, 512, 0)
    torch.cuda.synchronize()
    q = qkv[:, :H].float().reshape(B, S, nh, hd).transpose(1, 2).cpu()
    k = qkv[:, H:2 * H].float().reshape(B, S, nh, hd).transpose(1, 2).cpu()
    rq = O.apply_rope(q, cos, sin).transpose(1, 2).reshape(B * S, H)
    rk = O.apply_rope(k, cos, sin).transpose(1, 2).reshape(B * S, H)
    check(x[:, :H].cpu(), rq, 8e-3, "rope q")
    check(x[:, H:2 * H].cpu(), rk, 8e-3, "rope k")
    assert torch.equal(x[:, 2 * H:], qkv[:, 2 * H:])
    # backward = inverse rotation: applying it to the rotated tensor restores the input
    hip.call("vlr_rope", x, pos, cos_t, sin_t, B * S, H, hd, 3 * H, 512, 1)
    torch.cuda.synchronize()
    check(x, qkv, 1.5e-2, "rope bwd(fwd(x)) == x")


def test_swiglu_gelu_colsum_rows(hip):
    M, I = 123, 1384
    gu, dact = rnd(M, 2 * I, seed=1), rnd(M, I, seed=2)
    act = torch.empty(M, I, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_swiglu_fwd", gu, act, M, I)
    g = gu[:, :I].float().requires_grad_(True)
    u = gu[:, I:].float().requires_grad_(True)
    ref = F.silu(g) * u
    torch.cuda.synchronize()
    check(act, ref, 8e-3, "swiglu fwd")
    (ref * dact.float()).sum().backward()
    gu2 = gu.clone()
    hip.call("vlr_swiglu_bwd", gu2, dact, M, I)
    torch.cuda.synchronize()
    check(gu2[:, :I], g.grad, 8e-3, "swiglu dgate")
    check(gu2[:, I:], u.grad, 8e-3, "swiglu dup")
    z, dh = rnd(M, 1024, seed=3), rnd(M, 1024, seed=4)
    h = torch.empty_like(z)
    hip.call("vlr_gelu_fwd", z, h, z.numel())
    zf = z.float().requires_grad_(True)
    r = F.gelu(zf)
    (r * dh.float()).sum().backward()
    dz = torch.empty_like(z)
    hip.call("vlr_gelu_bwd", z, dh, dz, z.numel())
    torch.cuda.synchronize()
    check(h, r, 8e-3, "gelu fwd")
    check(dz, zf.grad, 8e-3, "gelu bwd")
    ws = torch.empty(hip.helper("vlr_colsum_workspace_bytes", 1024), dtype=torch.uint8, device=DEV)
    out = rnd(1024, seed=5)
    out0 = out.clone()
    hip.call("vlr_colsum", z, M, 1024, 1024, out, 1, ws)
    torch.cuda.synchronize()
    check(out, z.float().sum(0) + out0.float(), 8e-3, "colsum")
    rows = torch.tensor([5, 0, 77, 122], dtype=torch.int32, device=DEV)
    dst = torch.empty(4, 1024, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gather_rows", z, rows, dst, 4, 1024)
    back = torch.zeros_like(z)
    hip.call("vlr_scatter_rows", dst, rows, back, 4, 1024)
    v = torch.randn(1024, device=DEV)
    rd = torch.empty(M, device=DEV)
    hip.call("vlr_rowdot", z, v, rd, M, 1024)
    torch.cuda.synchronize()
    assert torch.equal(dst, z[rows.long()])
    assert torch.equal(back[rows.long()], z[rows.long()]) and float(back.abs().sum()) == float(z[rows.long()].abs().sum())
    check(rd, z.float() @ v, 1e-4, "rowdot")


# ---------------------------------------------------------------------------------------------------- attention
def ref_attention(q, k, v, causal, key_mask, scale):
    """q,k,v [B,nh,S,hd] fp32 -> out, probabilities (eager softmax, HF semantics)."""
    B, nh, S, hd = q.shape
    s = (q @ k.transpose(-1, -2)) * scale
    vis = torch.ones(S, S, dtype=torch.bool, device=q.device)
    if causal:
        vis = vis.tril()
    vis = vis[None, None].expand(B, 1, S, S)
    if key_mask is not None:
        vis = vis & (key_mask[:, None, None, :] != 0)
    s = s.masked_fill(~vis, float("-inf"))
    return torch.softmax(s, -1) @ v


@pytest.mark.parametrize("B,S,nh,hd,causal,masked", [
    (2, 64, 1, 128, True, False), (2, 200, 2, 128, True, True), (1, 831, 2, 128, True, True),
    (3, 577, 2, 64, False, False), (2, 100, 3, 64, False, False), (1, 129, 1, 128, False, False)])
def test_attention_fwd(hip, B, S, nh, hd, causal, masked):
    H = nh * hd
    qkv = rnd(B * S, 3 * H, seed=11, scale=1.0)
    km = None
    if masked:
        km = torch.ones(B, S, dtype=torch.int32, device=DEV)
        km[0, S - 13:] = 0                  # right padding
        if B > 1:
            km[1, S - 1:] = 0
    o = torch.full((B * S, H), float("nan"), dtype=torch.bfloat16, device=DEV)
    Sp = (S + 63) // 64 * 64
    lse = torch.zeros(B, nh, Sp, dtype=torch.float32, device=DEV)
    scale = 1.0 / math.sqrt(hd)
    hip.call("vlr_attn_fwd", qkv, qkv[:, H:], qkv[:, 2 * H:], 3 * H, o, H, lse, km, B, S, nh, hd, int(causal), scale)
    torch.cuda.synchronize()
    q, k, v = (qkv[:, i * H:(i + 1) * H].float().reshape(B, S, nh, hd).transpose(1, 2) for i in range(3))
    ref = ref_attention(q, k, v, causal, km, scale).transpose(1, 2).reshape(B * S, H)
    valid = torch.ones(B * S, dtype=torch.bool, device=DEV) if km is None else (km.reshape(-1) != 0)
    check(o[valid], ref[valid], 1.2e-2, "attention fwd")
    assert torch.isfinite(o.float()).all()
    # lse (log2 domain) against the reference logsumexp
    s = (q @ k.transpose(-1, -2)) * scale
    vis = torch.ones(S, S, dtype=torch.bool, device=DEV)
    if causal:
        vis = vis.tril()
    vis = vis[None, None].expand(B, 1, S, S)
    if km is not None:
        vis = vis & (km[:, None, None, :] != 0)
    l2 = torch.logsumexp(s.masked_fill(~vis, float("-inf")), -1) / math.log(2.0)
    check(lse[:, :, :S], l2, 2e-3, "lse")
    assert torch.isinf(lse[:, :, S:]).all()


def test_attention_left_padding_fully_masked_rows(hip):
    """leading padded keys (merge 'left padding'): queries that see no key give O = 0 and stay finite."""
    B, S, nh, hd = 1, 96, 1, 128
    H = nh * hd
    qkv = rnd(B * S, 3 * H, seed=5)
    km = torch.ones(B, S, dtype=torch.int32, device=DEV)
    km[0, :7] = 0
    o = torch.empty(B * S, H, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(B, nh, 128, dtype=torch.float32, device=DEV)
    hip.call("vlr_attn_fwd", qkv, qkv[:, H:], qkv[:, 2 * H:], 3 * H, o, H, lse, km, B, S, nh, hd, 1, 1 / math.sqrt(hd))
    torch.cuda.synchronize()
    assert torch.isfinite(o.float()).all() and float(o[:7].abs().max()) == 0.0
    q, k, v = (qkv[:, i * H:(i + 1) * H].float().reshape(B, S, nh, hd).transpose(1, 2) for i in range(3))
    ref = ref_attention(q, k, v, True, km, 1 / math.sqrt(hd)).transpose(1, 2).reshape(B * S, H)
    check(o[7:], ref[7:], 1.2e-2, "left-padded attention")


@pytest.mark.parametrize("B,S,nh,masked", [(1, 64, 1, False), (2, 200, 2, True), (1, 333, 1, True)])
def test_attention_bwd(hip, B, S, nh, masked):
    hd = 128
    H = nh * hd
    qkv = rnd(B * S, 3 * H, seed=21)
    do = rnd(B * S, H, seed=22)
    km = None
    if masked:
        km = torch.ones(B, S, dtype=torch.int32, device=DEV)
        km[0, S - 9:] = 0
        do[S - 9:S] = 0            # padded positions receive no gradient in the real step
    scale = 1.0 / math.sqrt(hd)
    Sp = (S + 63) // 64 * 64
    o = torch.empty(B * S, H, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(B, nh, Sp, dtype=torch.float32, device=DEV)
    hip.call("vlr_attn_fwd", qkv, qkv[:, H:], qkv[:, 2 * H:], 3 * H, o, H, lse, km, B, S, nh, hd, 1, scale)
    dqkv = torch.full((B * S, 3 * H), float("nan"), dtype=torch.bfloat16, device=DEV)
    delta = torch.zeros(B, nh, Sp, dtype=torch.float32, device=DEV)
    hip.call("vlr_attn_bwd", qkv, qkv[:, H:], qkv[:, 2 * H:], 3 * H, o, do, H, lse, delta, km, dqkv, dqkv[:, H:],
             dqkv[:, 2 * H:], 3 * H, B, S, nh, hd, 1, scale)
    torch.cuda.synchronize()
    x = qkv.float().requires_grad_(True)
    q, k, v = (x[:, i * H:(i + 1) * H].reshape(B, S, nh, hd).transpose(1, 2) for i in range(3))
    ref = ref_attention(q, k, v, True, km, scale).transpose(1, 2).reshape(B * S, H)
    (ref * do.float()).sum().backward()
    g = x.grad
    valid = torch.ones(B * S, dtype=torch.bool, device=DEV) if km is None else (km.reshape(-1) != 0)
    check(dqkv[valid][:, :H], g[valid][:, :H], 2e-2, "dq")
    check(dqkv[valid][:, H:2 * H], g[valid][:, H:2 * H], 2e-2, "dk")
    check(dqkv[valid][:, 2 * H:], g[valid][:, 2 * H:], 2e-2, "dv")
    assert torch.isfinite(dqkv.float()).all()
    if km is not None:   # padded keys get exactly zero dk / dv
        assert float(dqkv[~valid][:, H:].abs().max()) == 0.0


def test_attention_schedule_paths(hip):
    """80 K/V heads = 10 per XCD: bundles of 8 + a remainder bundle of 2 in the block order; 640 query blocks > the 512 resident
    workgroups: persistent forward on the ticket counters (twice, so the self-reset is exercised); right padding -> masked tiles in
    every kernel; the backward workspace arrives full of NaN (delta rows past S must come back as zeros: dS has no guard)."""
    B, S, nh, hd = 5, 900, 16, 128
    H = nh * hd
    qkv = rnd(B * S, 3 * H, seed=31)
    do = rnd(B * S, H, seed=32)
    km = torch.ones(B, S, dtype=torch.int32, device=DEV)
    km[0, S - 70:] = 0
    km[3, S - 5:] = 0
    do.view(B, S, H)[0, S - 70:] = 0
    do.view(B, S, H)[3, S - 5:] = 0
    scale = 1.0 / math.sqrt(hd)
    Sp = (S + 63) // 64 * 64
    lse = torch.zeros(B, nh, Sp, dtype=torch.float32, device=DEV)
    outs = []
    for _ in range(2):
        o = torch.full((B * S, H), float("nan"), dtype=torch.bfloat16, device=DEV)
        hip.call("vlr_attn_fwd", qkv, qkv[:, H:], qkv[:, 2 * H:], 3 * H, o, H, lse, km, B, S, nh, hd, 1, scale)
        outs.append(o)
    dqkv = torch.full((B * S, 3 * H), float("nan"), dtype=torch.bfloat16, device=DEV)
    delta = torch.full((B, nh, Sp), float("nan"), dtype=torch.float32, device=DEV)
    hip.call("vlr_attn_bwd", qkv, qkv[:, H:], qkv[:, 2 * H:], 3 * H, outs[0], do, H, lse, delta, km, dqkv, dqkv[:, H:],
             dqkv[:, 2 * H:], 3 * H, B, S, nh, hd, 1, scale)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    assert float(delta[:, :, S:].abs().max()) == 0.0 and torch.isfinite(delta).all()
    valid = km.reshape(-1) != 0
    g = torch.empty(B * S, 3 * H, device=DEV)
    ref = torch.empty(B * S, H, device=DEV)
    for b in range(B):                      # one sequence at a time: the eager reference holds S x S per head
        x = qkv[b * S:(b + 1) * S].float().requires_grad_(True)
        q, k, v = (x[:, i * H:(i + 1) * H].reshape(1, S, nh, hd).transpose(1, 2) for i in range(3))
        r = ref_attention(q, k, v, True, km[b:b + 1], scale).transpose(1, 2).reshape(S, H)
        (r * do[b * S:(b + 1) * S].float()).sum().backward()
        ref[b * S:(b + 1) * S] = r.detach()
        g[b * S:(b + 1) * S] = x.grad
    check(outs[0][valid], ref[valid], 1.2e-2, "attention fwd (persistent, bundled order)")
    check(dqkv[valid][:, :H], g[valid][:, :H], 2e-2, "dq")
    check(dqkv[valid][:, H:2 * H], g[valid][:, H:2 * H], 2e-2, "dk")
    check(dqkv[valid][:, 2 * H:], g[valid][:, 2 * H:], 2e-2, "dv")
    assert torch.isfinite(dqkv.float()).all()
    assert float(dqkv[~valid][:, H:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------- merge
def test_merge_matches_oracle(hip):
    H, P, V, image_token, model_pad = 64, 5, 90, 80, 81
    g = torch.Generator().manual_seed(3)
    Bh, T = 3, 12
    ids_h = torch.randint(3, 80, (Bh, T), generator=g)
    ids_h[:, 0] = 1
    for b in range(Bh):
        ids_h[b, 2 + b] = image_token
    # chosen / rejected halves share the prompt (and the image); ragged right padding with 0
    ids = torch.cat([ids_h, ids_h.clone()], 0)
    ids[Bh:, 8:] = torch.randint(3, 80, (Bh, T - 8), generator=g)
    am = torch.ones_like(ids)
    ids[1, 10:] = 0
    am[1, 10:] = 0
    ids[4, 9:] = 0
    am[4, 9:] = 0
    lab = ids.clone()
    lab[:, :6] = -100
    lab[am == 0] = -100
    table = rnd(V, H, seed=1)
    feats = rnd(Bh * P, H, seed=2)                     # deduplicated: one feature set per distinct image
    S = T - 1 + P
    Bn = 2 * Bh
    src = torch.empty(Bn, S, dtype=torch.int32, device=DEV)
    omask = torch.empty(Bn, S, dtype=torch.int32, device=DEV)
    olab = torch.empty(Bn, S, dtype=torch.int64, device=DEV)
    opos = torch.empty(Bn, S, dtype=torch.int32, device=DEV)
    imap = torch.empty(Bn, S, dtype=torch.uint8, device=DEV)
    inv = torch.empty(2, Bh * P, dtype=torch.int32, device=DEV)
    info = torch.zeros(2, dtype=torch.int32, device=DEV)
    idd, amd, labd = ids.to(DEV), am.to(DEV), lab.to(DEV)
    hip.call("vlr_merge_index", idd, amd, labd, Bn, T, S, P, image_token, model_pad, Bh * P, 2, src, omask, olab, opos, imap, inv, info)
    out = torch.empty(Bn, S, H, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_merge_fwd", src, idd, table, feats, out, Bn, T, S, H)
    torch.cuda.synchronize()
    f2 = torch.cat([feats, feats], 0).float().cpu().reshape(Bn, P, H)
    emb = table.float().cpu()[ids]
    e, m, l, p, mp = O.merge_input_ids_with_image_features(f2, emb, ids, am, lab, image_token, model_pad)
    assert int(info[0]) == Bn * P
    assert torch.equal(out.float().cpu(), e)
    assert torch.equal(omask.cpu().long(), m) and torch.equal(olab.cpu(), l) and torch.equal(opos.cpu().long(), p)
    assert torch.equal(imap.cpu().bool(), mp)
    # backward: d_feats sums the two halves, d_table scatter-adds duplicates
    dm = rnd(Bn, S, H, seed=4)
    dfe = torch.empty_like(feats)
    dtab = torch.zeros_like(table)
    hip.call("vlr_merge_bwd", dm, src, inv, idd, dfe, dtab, Bn, T, S, H, Bh * P, 2)
    torch.cuda.synchronize()
    embg = emb.clone().requires_grad_(True)
    fg = feats.float().cpu().clone().requires_grad_(True)
    e2, *_ = O.merge_input_ids_with_image_features(torch.cat([fg, fg], 0).reshape(Bn, P, H), embg, ids, am, lab, image_token, model_pad)
    (e2 * dm.float().cpu()).sum().backward()
    check(dfe.cpu(), fg.grad, 1e-2, "merge d_feats")
    tg = torch.zeros(V, H).index_add_(0, ids.reshape(-1), embg.grad.reshape(-1, H))
    check(dtab.cpu(), tg, 2e-2, "merge d_table")
    # a wrong image count is reported through info[0]
    info.zero_()
    hip.call("vlr_merge_index", idd, amd, labd, Bn, T, S, P, image_token, model_pad, (Bh - 1) * P, 2, src, omask, olab, opos, imap, inv, info)
    torch.cuda.synchronize()
    assert int(info[0]) != (Bh - 1) * P * 2


_MERGE_EMBED_CHILD = r"""
import os, sys, torch
root = sys.argv[1]
sys.path.insert(0, os.path.join(root, "vl-rlhf_amd"))
from vlrlhf import _hip
g = torch.Generator().manual_seed(11)
Bn, T, H = (int(x) for x in sys.argv[3:6])
P, V, image_token, pad = 20, 50, 48, 49
ids = torch.randint(0, 48, (Bn, T), generator=g)
ids[:, 5] = image_token
ids[1, T - 50:] = pad
am = (ids != pad).long()
lab = ids.clone()
S = T - 1 + P
dev = "cuda"
src = torch.empty(Bn, S, dtype=torch.int32, device=dev); omask = torch.empty(Bn, S, dtype=torch.int32, device=dev)
olab = torch.empty(Bn, S, dtype=torch.int64, device=dev); opos = torch.empty(Bn, S, dtype=torch.int32, device=dev)
imap = torch.empty(Bn, S, dtype=torch.uint8, device=dev); inv = torch.empty(1, Bn * P, dtype=torch.int32, device=dev)
info = torch.zeros(2, dtype=torch.int32, device=dev)
idd = ids.to(dev)
_hip.call("vlr_merge_index", idd, am.to(dev), lab.to(dev), Bn, T, S, P, image_token, pad, Bn * P, 1, src, omask, olab, opos, imap, inv, info)
dm = (torch.randn(Bn, S, H, generator=g) * 0.5).bfloat16().to(dev)
dtab = (torch.randn(V, H, generator=g) * 0.1).bfloat16().to(dev)       # read-modify-write: a non-zero table
_hip.call("vlr_merge_bwd", dm, src, inv, idd, None, dtab, Bn, T, S, H, Bn * P, 1)
torch.cuda.synchronize()
torch.save(dtab.cpu(), sys.argv[2])
"""


def test_merge_bwd_embed_lds_kernel_is_bit_identical_to_the_global_walk(hip, tmp_path):
    """merge_bwd_embed2_kernel (the positions' token ids in LDS, wave-level ballots) adds the same rows in the same order as
    merge_bwd_embed_kernel (VLR_MERGE_EMBED2=0, read once per process): 48 ids on 1276 positions - every id is held by dozens of
    positions in several 64-position groups and workgroups -, a padded tail, a non-zero table; and 19 352 positions (more than the 60 KiB
    of LDS a kernel gets without asking: the attribute path)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for shape in (("4", "300", "256"), ("8", "2400", "64")):
        outs = []
        for flag in ("1", "0"):
            f = str(tmp_path / f"dtab_{flag}_{shape[1]}.pt")
            r = subprocess.run([sys.executable, "-c", _MERGE_EMBED_CHILD, root, f, *shape], capture_output=True, text=True, timeout=600,
                               env=dict(os.environ, VLR_MERGE_EMBED2=flag))
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            outs.append(torch.load(f))
        assert torch.equal(outs[0], outs[1])
        assert float(outs[0].float().abs().max()) > 1.0       # dozens of rows were added per id


# ---------------------------------------------------------------------------------------------------- logps / loss
@pytest.mark.parametrize("average", [0, 1])
def test_logps_pipeline(hip, average):
    Bn, S, V = 4, 37, 264
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(Bn, S, V, generator=g) * 3
    labels = torch.randint(0, V, (Bn, S), generator=g)
    labels[:, :9] = -100
    labels[1, 30:] = -100
    labels[3, 20:] = -100
    ref = O.get_batch_logps(logits, labels, average_log_prob=bool(average))
    ld, lb = logits.to(DEV), labels.to(DEV)
    rows = torch.empty(Bn * S, dtype=torch.int32, device=DEV)
    tgt = torch.empty(Bn * S, dtype=torch.int32, device=DEV)
    seq_off = torch.empty(Bn + 1, dtype=torch.int32, device=DEV)
    hip.call("vlr_build_rows", lb, None, Bn, S, -100, rows, tgt, seq_off)
    torch.cuda.synchronize()
    R = int(seq_off[-1])
    mask = labels[:, 1:] != -100
    assert R == int(mask.sum())
    exp_rows = torch.nonzero(F.pad(mask, (0, 1)).reshape(-1)).squeeze(1)
    assert torch.equal(rows[:R].cpu().long(), exp_rows)
    tok = torch.empty(R, device=DEV)
    lse = torch.empty(R, device=DEV)
    hip.call("vlr_logp_rows", ld, rows, tgt, R, V, V, tok, lse)
    out = torch.empty(Bn, device=DEV)
    hip.call("vlr_seq_sum", tok, seq_off, Bn, average, out)
    torch.cuda.synchronize()
    assert torch.allclose(out.cpu(), ref, rtol=1e-5, atol=1e-4)
    # backward: d logits
    lg = logits.clone().requires_grad_(True)
    dl_up = torch.randn(Bn, generator=g)
    (O.get_batch_logps(lg, labels, average_log_prob=bool(average)) * dl_up).sum().backward()
    compact = ld.reshape(-1, V)[rows[:R].long()].contiguous()
    dlog = torch.empty(R, V, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_dlogits_rows", compact, tgt, lse, seq_off, Bn, dl_up.to(DEV), average, R, V, V, dlog, V)
    torch.cuda.synchronize()
    check(dlog.cpu(), lg.grad.reshape(-1, V)[exp_rows], 8e-3, "dlogits")


def test_ddpo_shared_mask_rows(hip):
    Bn, S = 4, 20
    g = torch.Generator().manual_seed(2)
    labels = torch.randint(3, 30, (Bn, S), generator=g)
    labels[2] = labels[0]
    labels[2, 12:15] = torch.tensor([31, 32, 33])
    labels[:, :6] = -100
    shared = O.ddpo_shared_mask(labels)
    rows = torch.empty(Bn * S, dtype=torch.int32, device=DEV)
    tgt = torch.empty(Bn * S, dtype=torch.int32, device=DEV)
    seq_off = torch.empty(Bn + 1, dtype=torch.int32, device=DEV)
    hip.call("vlr_build_rows", labels.to(DEV), shared.to(torch.uint8).to(DEV), Bn, S, -100, rows, tgt, seq_off)
    torch.cuda.synchronize()
    keep = (labels[:, 1:] != -100) & shared
    assert seq_off.cpu().tolist() == [0] + torch.cumsum(keep.sum(-1), 0).tolist()


LOSS_IDS = {"sigmoid": 0, "ddpo": 0, "hinge": 1, "ipo": 2, "kto_pair": 3}


@pytest.mark.parametrize("loss_type", list(LOSS_IDS))
@pytest.mark.parametrize("ls,rf", [(0.0, False), (0.2, True)])
def test_dpo_loss_fwd_bwd(hip, loss_type, ls, rf):
    n, beta = 6, 0.3
    g = torch.Generator().manual_seed(7)
    pc, pr, rc, rr = [(torch.randn(n, generator=g) * 4 - 30) for _ in range(4)]
    pcg, prg = pc.clone().requires_grad_(True), pr.clone().requires_grad_(True)
    losses, cr, rw = O.dpo_loss(pcg, prg, rc, rr, beta, ls, loss_type, rf)
    losses.mean().backward()
    nl = losses.numel()
    d = [t.to(DEV) for t in (pc, pr, rc, rr)]
    out_l = torch.empty(nl, device=DEV)
    out = [torch.empty(n, device=DEV) for _ in range(4)]
    mean = torch.empty(1, device=DEV)
    hip.call("vlr_dpo_loss", *d, n, beta, ls, LOSS_IDS[loss_type], int(rf), out_l, out[0], out[1], out[2], out[3], mean, None)
    torch.cuda.synchronize()
    assert torch.allclose(out_l.cpu(), losses.detach(), rtol=2e-5, atol=2e-6)
    assert torch.allclose(out[0].cpu(), cr, rtol=1e-5, atol=1e-6) and torch.allclose(out[1].cpu(), rw, rtol=1e-5, atol=1e-6)
    assert torch.allclose(out[2].cpu(), pcg.grad, rtol=2e-4, atol=2e-7), (out[2].cpu(), pcg.grad)
    assert torch.allclose(out[3].cpu(), prg.grad, rtol=2e-4, atol=2e-7)
    assert abs(float(mean) - float(losses.mean())) < 2e-5 * abs(float(losses.mean())) + 1e-6
    # arbitrary upstream gradient
    up = torch.randn(nl, generator=g)
    pcg.grad = prg.grad = None
    (O.dpo_loss(pcg, prg, rc, rr, beta, ls, loss_type, rf)[0] * up).sum().backward()
    hip.call("vlr_dpo_loss", *d, n, beta, ls, LOSS_IDS[loss_type], int(rf), out_l, out[0], out[1], out[2], out[3], mean, up.to(DEV))
    torch.cuda.synchronize()
    assert torch.allclose(out[2].cpu(), pcg.grad, rtol=2e-4, atol=2e-6)
    assert torch.allclose(out[3].cpu(), prg.grad, rtol=2e-4, atol=2e-6)


def test_dpo_loss_unknown_type(hip):
    t = torch.zeros(2, device=DEV)
    with pytest.raises(ValueError, match="Unknown loss type"):
        hip.call("vlr_dpo_loss", t, t, t, t, 2, 0.1, 0.0, 9, 0, t, t, t, t, t, t, None)


# ---------------------------------------------------------------------------------------------------- optimizer
def test_sqnorm_clip_adamw(hip):
    n = 8 * 3001
    g = torch.Generator().manual_seed(1)
    w = torch.randn(n, generator=g)
    grads = (torch.randn(n, generator=g) * 0.01).bfloat16()
    ws = torch.empty(hip.helper("vlr_grad_sqnorm_workspace_bytes"), dtype=torch.uint8, device=DEV)
    out3 = torch.zeros(3, device=DEV)
    gd = grads.to(DEV)
    hip.call("vlr_grad_sqnorm", gd, n, 1.0, 1.0, 0.0, ws, out3)
    torch.cuda.synchronize()
    total = float(grads.float().norm())
    assert abs(float(out3[0]) - total) < 1e-4 * total
    assert abs(float(out3[1]) - min(1.0, 1.0 / (total + 1e-6))) < 1e-5
    W = {"a.weight": w.clone()}
    G = {"a.weight": grads.float().clone()}
    tot = O.clip_grad_norm_(G, 1.0)
    state = {}
    master, m, v = w.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    p16 = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    hp = dict(lr=1e-3, beta1=0.9, beta2=0.98, eps=1e-6, weight_decay=0.05)
    for step in (1, 2, 3):
        O.adamw_step(W, G, state, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"])
        hip.call("vlr_adamw_step", master, m, v, gd, p16, n, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"], step, out3)
    torch.cuda.synchronize()
    assert float((master.cpu() - W["a.weight"]).abs().max()) < 3e-6
    assert torch.equal(p16.cpu(), master.cpu().bfloat16())
    assert abs(float(tot) - total) < 1e-4 * total


# ---------------------------------------------------------------------------------------------------- composed layer
def test_decoder_layer_fwd_bwd_vs_oracle(hip):
    """One LLaMA layer through vlr_decoder_layer_fwd/bwd against the CPU oracle with bf16 rounding emulated at the
    same points, and against fp32 autograd for the gradients."""
    from vlrlhf import _hip as HH
    B, S, nh, hd, I = 2, 70, 2, 128, 384
    H = nh * hd
    M = B * S
    cfgo = dict(hidden=H, inter=I, layers=1, heads=nh, vocab=8, rms_eps=1e-5)
    g = torch.Generator().manual_seed(0)
    W = {}
    p = "language_model.model.layers.0."
    for nm, shp in (("self_attn.q_proj", (H, H)), ("self_attn.k_proj", (H, H)), ("self_attn.v_proj", (H, H)),
                    ("self_attn.o_proj", (H, H)), ("mlp.gate_proj", (I, H)), ("mlp.up_proj", (I, H)), ("mlp.down_proj", (H, I))):
        W[p + nm + ".weight"] = (torch.randn(*shp, generator=g) * 0.05).bfloat16().float()
    W[p + "input_layernorm.weight"] = (1 + 0.1 * torch.randn(H, generator=g)).bfloat16().float()
    W[p + "post_attention_layernorm.weight"] = (1 + 0.1 * torch.randn(H, generator=g)).bfloat16().float()
    W["language_model.model.norm.weight"] = torch.ones(H)
    x = (torch.randn(B, S, H, generator=g)).bfloat16().float()
    am = torch.ones(B, S, dtype=torch.long)
    am[1, S - 6:] = 0
    pos = (am.cumsum(-1) - 1).masked_fill(am == 0, 1)
    dy = torch.randn(B, S, H, generator=g).bfloat16().float()
    dy[am == 0] = 0
    # oracle: fp32 autograd of the bf16-emulated forward (rounding is piecewise constant -> straight-through not needed
    # for the fp32 reference gradient; use the un-rounded forward for gradients)
    leaves = {k: v.clone().requires_grad_(True) for k, v in W.items()}
    xg = x.clone().requires_grad_(True)
    col = []
    O.llama_hidden(xg, am, pos, leaves, cfgo, emulate_bf16=False, collect=col)
    (col[0] * dy).sum().backward()
    col16 = []
    with torch.no_grad():
        O.llama_hidden(x, am, pos, W, cfgo, emulate_bf16=True, collect=col16)

    def dv(t, dt=torch.bfloat16):
        return t.to(dt).to(DEV).contiguous()

    wqkv = dv(torch.cat([W[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], 0))
    wgu = dv(torch.cat([W[p + "mlp.gate_proj.weight"], W[p + "mlp.up_proj.weight"]], 0))
    wo, wdown = dv(W[p + "self_attn.o_proj.weight"]), dv(W[p + "mlp.down_proj.weight"])
    ln1, ln2 = dv(W[p + "input_layernorm.weight"]), dv(W[p + "post_attention_layernorm.weight"])
    cos_t = torch.empty(256, hd // 2, device=DEV)
    sin_t = torch.empty_like(cos_t)
    hip.call("vlr_rope_table", cos_t, sin_t, 256, hd, 10000.0)
    cfg = HH.LlamaCfg(H, I, nh, hd, 1e-5, 256, cos_t.data_ptr(), sin_t.data_ptr())
    lw = HH.LayerWeights(*(t.data_ptr() for t in (ln1, wqkv, wo, ln2, wgu, wdown)))
    Sp = (S + 63) // 64 * 64
    bufs = dict(xn1=torch.empty(M, H), rstd1=torch.empty(M, dtype=torch.float32), qkv=torch.empty(M, 3 * H), attn=torch.empty(M, H),
                lse=torch.zeros(B, nh, Sp, dtype=torch.float32), x_mid=torch.empty(M, H), xn2=torch.empty(M, H),
                rstd2=torch.empty(M, dtype=torch.float32), gu=torch.empty(M, 2 * I), act=torch.empty(M, I), x_out=torch.empty(M, H))
    bufs = {k: (v.to(DEV) if v.dtype == torch.float32 and k in ("rstd1", "rstd2", "lse") else v.bfloat16().to(DEV)) for k, v in bufs.items()}
    la = HH.LayerActs(*(bufs[k].data_ptr() for k in ("xn1", "rstd1", "qkv", "attn", "lse", "x_mid", "xn2", "rstd2", "gu", "act", "x_out")))
    xin = dv(x.reshape(M, H))
    posd = pos.to(torch.int32).to(DEV)
    kmd = am.to(torch.int32).to(DEV)
    hip.call("vlr_decoder_layer_fwd", cfg, lw, la, xin, posd, kmd, B, S)
    torch.cuda.synchronize()
    valid = (am.reshape(-1) != 0)
    check(bufs["x_out"].cpu()[valid], col16[0].reshape(M, H)[valid], 2e-2, "layer fwd vs bf16-emulated oracle")
    check(bufs["x_out"].cpu()[valid], col[0].detach().reshape(M, H)[valid], 3e-2, "layer fwd vs fp32 oracle")
    # backward
    grads = {k: torch.full_like(t, float("nan")) for k, t in dict(ln1=ln1, wqkv=wqkv, wo=wo, ln2=ln2, wgu=wgu, wdown=wdown).items()}
    lg = HH.LayerGrads(*(grads[k].data_ptr() for k in ("ln1", "wqkv", "wo", "ln2", "wgu", "wdown")))
    wsb = dict(dact=torch.empty(M, I), dxn=torch.empty(M, H), dattn=torch.empty(M, H), dqkv=torch.empty(M, 3 * H), dx_mid=torch.empty(M, H))
    wsb = {k: v.bfloat16().to(DEV) for k, v in wsb.items()}
    delta = torch.zeros(B, nh, Sp, dtype=torch.float32, device=DEV)
    nws = torch.empty(hip.helper("vlr_rmsnorm_bwd_workspace_bytes", H), dtype=torch.uint8, device=DEV)
    lws = HH.LayerBwdWs(wsb["dact"].data_ptr(), wsb["dxn"].data_ptr(), wsb["dattn"].data_ptr(), wsb["dqkv"].data_ptr(),
                        wsb["dx_mid"].data_ptr(), delta.data_ptr(), nws.data_ptr())
    dxin = torch.empty(M, H, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_decoder_layer_bwd", cfg, lw, lg, 0, la, lws, xin, dv(dy.reshape(M, H)), dxin, posd, kmd, B, S)
    torch.cuda.synchronize()
    check(dxin.cpu()[valid], xg.grad.reshape(M, H)[valid], 4e-2, "layer dx")
    gq = torch.cat([leaves[p + f"self_attn.{n}_proj.weight"].grad for n in "qkv"], 0)
    ggu = torch.cat([leaves[p + "mlp.gate_proj.weight"].grad, leaves[p + "mlp.up_proj.weight"].grad], 0)
    check(grads["wqkv"].cpu(), gq, 4e-2, "dWqkv")
    check(grads["wo"].cpu(), leaves[p + "self_attn.o_proj.weight"].grad, 4e-2, "dWo")
    check(grads["wgu"].cpu(), ggu, 4e-2, "dWgu")
    check(grads["wdown"].cpu(), leaves[p + "mlp.down_proj.weight"].grad, 4e-2, "dWdown")
    check(grads["ln1"].cpu(), leaves[p + "input_layernorm.weight"].grad, 4e-2, "dln1")
    check(grads["ln2"].cpu(), leaves[p + "post_attention_layernorm.weight"].grad, 4e-2, "dln2")


@pytest.mark.parametrize("shape", [(4096, 128, 12792), (384, 4096, 12792), (128, 11008, 6000), (256, 64, 2048)])
def test_gemm_tn_split_k(hip, shape):
    """weight-gradient-shaped skinny problems (LoRA dB / dA): few output tiles, reduction over all tokens -> split-K."""
    M, N, K = shape
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=DEV)
    assert hip.helper("vlr_gemm_set_splitk_workspace", ws.data_ptr(), ws.numel()) == 0
    try:
        a = rnd(K, M, seed=1, scale=0.5)          # TN: A stored [K][M], B stored [K][N]
        b = rnd(K, N, seed=2, scale=0.5)
        ref = a.float().t() @ b.float()
        c = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        hip.call("vlr_gemm_bf16", 2, a, b, c, None, None, M, N, K, M, N, N, 0, 0, 0, 0)
        check(c, ref, 8e-3, f"split-K {shape}")
        c0 = rnd(M, N, seed=3)
        c1 = c0.clone()
        hip.call("vlr_gemm_bf16_scaled", 2, a, b, c1, None, None, M, N, K, M, N, N, 0, 0, 1, 0, 0.25)
        check(c1, c0.float() + 0.25 * ref, 8e-3, f"split-K accumulate+alpha {shape}")
        cf = torch.empty(M, N, dtype=torch.float32, device=DEV)
        hip.call("vlr_gemm_bf16", 2, a, b, cf, None, None, M, N, K, M, N, N, 0, 0, 0, 1)
        check(cf, ref, 2e-3, f"split-K fp32 out {shape}")
        # the un-split kernel gives the same answer
        assert hip.helper("vlr_gemm_set_splitk_workspace", None, 0) == 0
        c2 = torch.empty_like(c)
        hip.call("vlr_gemm_bf16", 2, a, b, c2, None, None, M, N, K, M, N, N, 0, 0, 0, 0)
        check(c2, c, 4e-3, "split vs un-split")
    finally:
        hip.ensure_splitk_workspace(force=True)


@pytest.mark.parametrize("layout", [0, 1])
def test_gemm_peeled_rows_split_k(hip, layout):
    """12792 rows = 48 full 256-row tile rows (three whole rounds of 256x256 tiles) + 504 peeled rows that run as 128x128
    tiles split along K, reduced by the kernel that applies bias / residual / accumulate."""
    hip.ensure_splitk_workspace(force=True)
    M, N, K = 12792, 4096, 4352
    a = rnd(M, K, seed=1, scale=0.5)
    b = rnd(N, K, seed=2, scale=0.5)
    bias = rnd(N, seed=3)
    res = rnd(M, N, seed=4)
    c0 = rnd(M, N, seed=5)
    ref = a.float() @ b.float().t() * 0.5 + bias.float() + res.float() + c0.float()
    Bm = b if layout == 0 else b.t().contiguous()
    c = c0.clone()
    hip.call("vlr_gemm_bf16_scaled", layout, a, Bm, c, bias, res, M, N, K, K, K if layout == 0 else N, N, N, 0, 1, 0, 0.5)
    check(c, ref, 8e-3, f"peel + split-K layout {layout}")
    check(c[-504:], ref[-504:], 8e-3, "peeled rows")


@pytest.mark.parametrize("shape", [(3592, 3336, 192), (4344, 4352, 256)])
@pytest.mark.parametrize("layout", [0, 2])
def test_gemm_accumulate_odd_tile_counts(hip, layout, shape):
    """210 tiles (one per workgroup) and 289 tiles (persistent workgroups, 289 % 8 = 1): every tile is computed exactly once -
    a tile visited twice would show up as a doubled accumulate."""
    M, N, K = shape
    a = rnd(M, K, seed=1, scale=0.5)
    b = rnd(N, K, seed=2, scale=0.5)
    c0 = rnd(M, N, seed=3)
    ref = c0.float() + a.float() @ b.float().t()
    A = a if layout != 2 else a.t().contiguous()
    Bm = b if layout == 0 else b.t().contiguous()
    c = c0.clone()
    hip.call("vlr_gemm_bf16", layout, A, Bm, c, None, None, M, N, K, K if layout != 2 else M, K if layout == 0 else N, N, 0, 0, 1, 0)
    check(c, ref, 8e-3, f"accumulate {shape} layout {layout}")


@pytest.mark.parametrize("M,D", [(1024, 4096), (300, 256), (37, 1664)])
def test_layernorm_bwd(hip, M, D):
    """vlr_layernorm_bwd (statistics recomputed from x) against torch autograd of F.layer_norm, with and without accumulation"""
    x = rnd(M, D, seed=1)
    w, b = (1 + 0.1 * torch.randn(D)).bfloat16().to(DEV), (0.1 * torch.randn(D)).bfloat16().to(DEV)
    dy = rnd(M, D, seed=2)
    xf, wf, bf = x.float().requires_grad_(True), w.float().requires_grad_(True), b.float().requires_grad_(True)
    F.layer_norm(xf, (D,), wf, bf, 1e-6).backward(dy.float())
    ws = torch.empty(hip.helper("vlr_layernorm_bwd_workspace_bytes", D), dtype=torch.uint8, device=DEV)
    dx = torch.empty_like(x)
    dw, db = torch.full((D,), 0.5, dtype=torch.bfloat16, device=DEV), torch.zeros(D, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_layernorm_bwd", dy, x, w, 1e-6, dx, dw, db, 0, ws, M, D)
    torch.cuda.synchronize()
    check(dx, xf.grad, 8e-3, "ln dx")
    check(dw, wf.grad, 8e-3, "ln dw")
    check(db, bf.grad, 8e-3, "ln db")
    hip.call("vlr_layernorm_bwd", dy, x, w, 1e-6, None, dw, db, 1, ws, M, D)      # accumulate, no dx
    torch.cuda.synchronize()
    check(dw, 2 * wf.grad, 1.2e-2, "ln dw accumulate")


# ---------------------------------------------------------------------------------------------------- fused epilogues
@pytest.mark.parametrize("shape", [(4104, 2176, 512), (4352, 2184, 320), (12792, 2048, 256), (300, 256, 128)])
@pytest.mark.parametrize("store_gu", [1, 0])
def test_gemm_swiglu_fused(hip, shape, store_gu):
    """vlr_gemm_swiglu: act = silu(x Wg^T) * (x Wu^T) from the fp32 accumulators; shapes with > 256 workgroup tiles take the
    fused 256-tile kernel (ragged M, I not a multiple of 128, a peeled tail), the last one the plain GEMM + SwiGLU kernel."""
    M, I, K = shape
    x = rnd(M, K, seed=1)
    w = rnd(2 * I, K, scale=0.05, seed=2)
    gu_ref = x.float() @ w.float().t()
    act_ref = F.silu(gu_ref[:, :I]) * gu_ref[:, I:]
    gu = torch.full((M, 2 * I), float("nan"), dtype=torch.bfloat16, device=DEV)
    act = torch.full((M, I), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_swiglu", x, w, gu, act, M, I, K, K, store_gu)
    torch.cuda.synchronize()
    check(act, act_ref, 8e-3, f"swiglu act {shape}")
    if store_gu:
        check(gu, gu_ref, 8e-3, f"swiglu gate|up {shape}")
    # the unfused path (plain GEMM, then the SwiGLU kernel on the rounded gate|up) agrees to bf16 rounding
    gu2 = torch.empty_like(gu)
    act2 = torch.empty_like(act)
    hip.call("vlr_gemm_bf16", 0, x, w, gu2, None, None, M, 2 * I, K, K, K, 2 * I, 0, 0, 0, 0)
    hip.call("vlr_swiglu_fwd", gu2, act2, M, I)
    torch.cuda.synchronize()
    check(act, act2, 1.6e-2, f"fused vs unfused {shape}")


@pytest.mark.parametrize("shape", [(4104, 512, 12, 12), (6400, 320, 16, 4), (12792, 256, 8, 8), (300, 128, 2, 2)])
def test_gemm_qkv_rope_fused(hip, shape):
    """vlr_gemm_qkv_rope: q|k|v projection with rotate-half RoPE in the epilogue (q and k heads only; grouped-query layouts have
    fewer k/v heads), against the fp32 reference rotation of the fp32 product."""
    M, K, nh, nkv = shape
    hd = 128
    N, rope_cols = (nh + 2 * nkv) * hd, (nh + nkv) * hd
    max_pos = 700
    x = rnd(M, K, seed=3)
    w = rnd(N, K, scale=0.05, seed=4)
    g = torch.Generator().manual_seed(5)
    pos = torch.randint(0, max_pos, (M,), generator=g, dtype=torch.int32).to(DEV)
    cos = torch.empty(max_pos, hd // 2, dtype=torch.float32, device=DEV)
    sin = torch.empty_like(cos)
    hip.call("vlr_rope_table", cos, sin, max_pos, hd, 10000.0)
    y = (x.float() @ w.float().t())
    ref = y.clone()
    heads = y[:, :rope_cols].view(M, nh + nkv, hd)
    c, s_ = cos[pos.long()][:, None, :], sin[pos.long()][:, None, :]
    x1, x2 = heads[..., : hd // 2], heads[..., hd // 2:]
    ref[:, :rope_cols] = torch.cat([x1 * c - x2 * s_, x2 * c + x1 * s_], -1).reshape(M, rope_cols)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_qkv_rope", x, w, out, pos, cos, sin, M, N, rope_cols, K, K, hd, max_pos)
    torch.cuda.synchronize()
    check(out, ref, 8e-3, f"qkv rope {shape}")
    assert torch.isfinite(out.float()).all()
    # biased projection (Qwen c_attn): the bias enters before the rotation
    bias = rnd(N, scale=0.5, seed=9)
    yb = y + bias.float()
    refb = yb.clone()
    hb = yb[:, :rope_cols].view(M, nh + nkv, hd)
    b1, b2 = hb[..., : hd // 2], hb[..., hd // 2:]
    refb[:, :rope_cols] = torch.cat([b1 * c - b2 * s_, b2 * c + b1 * s_], -1).reshape(M, rope_cols)
    out.fill_(float("nan"))
    hip.call("vlr_gemm_qkv_rope_bias", x, w, bias, out, pos, cos, sin, M, N, rope_cols, K, K, hd, max_pos)
    torch.cuda.synchronize()
    check(out, refb, 8e-3, f"qkv rope bias {shape}")


# ---------------------------------------------------------------------------------------------------- LoRA adapter segment
def _blockdiag_add(y, u, Bl, r, bounds):
    """y[:, block t] += u[:, t*r:(t+1)*r] Bl[block t rows]^T (fp32)"""
    lo = 0
    for t, hi in enumerate(bounds):
        y[:, lo:hi] += u[:, t * r:(t + 1) * r].float() @ Bl[lo:hi].float().t()
        lo = hi
    return y


@pytest.mark.parametrize("shape", [(4352, 4352, 512, 128, True), (12792, 4096, 256, 64, True), (4104, 4360, 320, 24, False), (300, 256, 128, 16, True)])
def test_gemm_lora_segment(hip, shape):
    """vlr_gemm_lora: y = x W^T + u Bl^T (+ residual) in ONE K loop (the adapter operands are a second segment of the reduction);
    big shapes run the persistent segment kernel (asserted: > 256 tiles; ragged M / N, r not a multiple of the 64-wide K tile, a
    peeled tail), the small one base GEMM + skinny GEMM."""
    M, N, K, r, res = shape
    assert M < 1000 or ((M + 255) // 256) * ((N + 255) // 256) > 256
    x, W = rnd(M, K, seed=1), rnd(N, K, scale=0.05, seed=2)
    ldu = 7 * r                                        # u sits inside the layer's [M][7r] buffer
    ubuf = rnd(M, ldu, scale=0.5, seed=3)
    u = ubuf[:, 3 * r:4 * r]
    Bl = rnd(N, r, scale=0.05, seed=4)
    resid = rnd(M, N, seed=5) if res else None
    ref = _blockdiag_add(x.float() @ W.float().t(), u, Bl, r, [N])
    if res:
        ref = ref + resid.float()
    y = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_lora", x, K, W, y, N, resid, N, M, N, K, u, ldu, Bl, r)
    torch.cuda.synchronize()
    check(y, ref, 8e-3, f"gemm_lora {shape}")


@pytest.mark.parametrize("shape", [(4352, 2176, 512, 128), (4104, 2184, 320, 40), (12792, 2048, 256, 64), (300, 256, 128, 16)])
def test_gemm_swiglu_lora_segment(hip, shape):
    """vlr_gemm_swiglu_lora: gate and up take DIFFERENT adapter inputs (u_gate | u_up); the gate half of a tile reads zeros over the
    up adapter's K range and vice versa."""
    M, I, K, r = shape
    x, w = rnd(M, K, seed=1), rnd(2 * I, K, scale=0.05, seed=2)
    u = rnd(M, 2 * r, scale=0.5, seed=3)
    Bl = rnd(2 * I, r, scale=0.05, seed=4)
    gu_ref = _blockdiag_add(x.float() @ w.float().t(), u, Bl, r, [I, 2 * I])
    act_ref = F.silu(gu_ref[:, :I]) * gu_ref[:, I:]
    gu = torch.full((M, 2 * I), float("nan"), dtype=torch.bfloat16, device=DEV)
    act = torch.full((M, I), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_swiglu_lora", x, w, gu, act, M, I, K, K, u, 2 * r, Bl, r)
    torch.cuda.synchronize()
    check(gu, gu_ref, 8e-3, f"swiglu lora gate|up {shape}")
    check(act, act_ref, 8e-3, f"swiglu lora act {shape}")


@pytest.mark.parametrize("shape", [(4104, 512, 12, 12, 128), (6400, 320, 16, 4, 64), (12792, 256, 8, 8, 32), (300, 128, 2, 2, 16)])
def test_gemm_qkv_rope_lora_segment(hip, shape):
    """vlr_gemm_qkv_rope_lora: three adapters (q, k, v; grouped-query widths) + RoPE in the epilogue of one GEMM"""
    M, K, nh, nkv, r = shape
    hd = 128
    Nq, Nkv = nh * hd, nkv * hd
    N, rope_cols = Nq + 2 * Nkv, Nq + Nkv
    max_pos = 700
    x, w = rnd(M, K, seed=3), rnd(N, K, scale=0.05, seed=4)
    u = rnd(M, 3 * r, scale=0.5, seed=6)
    Bl = rnd(N, r, scale=0.05, seed=7)
    pos = torch.randint(0, max_pos, (M,), generator=torch.Generator().manual_seed(5), dtype=torch.int32).to(DEV)
    cos = torch.empty(max_pos, hd // 2, dtype=torch.float32, device=DEV)
    sin = torch.empty_like(cos)
    hip.call("vlr_rope_table", cos, sin, max_pos, hd, 10000.0)
    y = _blockdiag_add(x.float() @ w.float().t(), u, Bl, r, [Nq, Nq + Nkv, N])
    ref = y.clone()
    heads = y[:, :rope_cols].view(M, nh + nkv, hd)
    c, s_ = cos[pos.long()][:, None, :], sin[pos.long()][:, None, :]
    x1, x2 = heads[..., : hd // 2], heads[..., hd // 2:]
    ref[:, :rope_cols] = torch.cat([x1 * c - x2 * s_, x2 * c + x1 * s_], -1).reshape(M, rope_cols)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_qkv_rope_lora", x, w, None, out, pos, cos, sin, M, N, rope_cols, K, K, hd, max_pos, u, 3 * r, Bl, r, Nq, Nkv)
    torch.cuda.synchronize()
    check(out, ref, 8e-3, f"qkv rope lora {shape}")


@pytest.mark.parametrize("keep", [64, 0])
def test_adapter_segment_row_tile_skip(hip, keep):
    """vlr_gemm_seg_rowskip / vlr_rows_tile_flags (ABI v8): 256-row tiles without a marked row run only the first `keep` K elements of every
    sub-target's block of the adapter segment ([u_lora 64 | u_plora 128] per sub-target here; keep = 0: the whole segment is skipped - PLoRA
    alone).  The rest of u is zero on those rows by contract, so the result is BIT-IDENTICAL to the full segment; NaNs planted in that
    part of u on the flagged tiles prove that it is not read there (without the flags they come out).  All three fused entry points;
    ragged M (a partial last tile), a peeled tail included."""
    from vlrlhf import _hip as HH
    HH.ensure_splitk_workspace(DEV, force=True)
    rl, rp = (64, 128) if keep else (0, 192)
    R = rl + rp
    M, K, hd = 12792, 512, 128                      # 50 row tiles
    g = torch.Generator().manual_seed(3)
    marked = torch.zeros(M, dtype=torch.uint8)
    for t in range(0, 50, 3):                       # tiles 0, 3, 6, ... hold marked rows (a run in the middle of the tile)
        marked[t * 256 + 40: t * 256 + 200] = 1
    marked[49 * 256 + 5] = 1                        # the partial last tile is marked too
    marked = marked.to(DEV)
    flags = torch.full((50,), 7, dtype=torch.uint8, device=DEV)
    hip.call("vlr_rows_tile_flags", marked, M, 256, flags)
    torch.cuda.synchronize()
    want_flags = torch.tensor([0 if (t % 3 == 0 or t == 49) else 1 for t in range(50)], dtype=torch.uint8)
    assert torch.equal(flags.cpu(), want_flags)
    rows_flagged = (want_flags.repeat_interleave(256)[:M] == 1).to(DEV)

    def make_u(nsub, poison):
        u = rnd(M, nsub * R, scale=0.5, seed=11)
        for t in range(nsub):
            blk = u[:, t * R + rl:(t + 1) * R]
            blk[marked == 0] = 0                     # the row-restricted adapter's block: zero on the unmarked rows
            if poison:
                blk[rows_flagged] = float("nan")     # ... and poisoned where the kernel must not look
        return u

    def run(fn, nsub):
        outs = []
        for poison, use_flags in ((False, False), (False, True), (True, True), (True, False)):
            u = make_u(nsub, poison)
            assert hip.helper("vlr_gemm_seg_rowskip", flags.data_ptr() if use_flags else None, keep) == 0
            outs.append(fn(u))
            torch.cuda.synchronize()
        full, skip, skip_poisoned, noskip_poisoned = outs
        for a_, b_, c_ in zip(full, skip, skip_poisoned):
            assert torch.isfinite(a_.float()).all()
            assert torch.equal(a_, b_), "row-tile skip changed the result"
            assert torch.equal(a_, c_), "the skipped part of u was read"
        assert not all(torch.isfinite(t_.float()).all() for t_ in noskip_poisoned), "the poison never reached a kernel: the test proves nothing"

    # plain + residual (bf16) and fp32 residual stream
    N = 4352
    x, W, Bl = rnd(M, K, seed=1), rnd(N, K, scale=0.05, seed=2), rnd(N, R, scale=0.05, seed=4)
    resid = rnd(M, N, seed=5, dtype=torch.float32)

    def f_lora(u):
        y = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
        hip.call("vlr_gemm_lora_f32res", x, K, W, y, N, resid, N, M, N, K, u, R, Bl, R)
        return (y,)
    run(f_lora, 1)
    # SwiGLU: two sub-targets (gate, up)
    I = 2176
    wgu, Bgu = rnd(2 * I, K, scale=0.05, seed=6), rnd(2 * I, R, scale=0.05, seed=7)

    def f_swiglu(u):
        gu = torch.full((M, 2 * I), float("nan"), dtype=torch.bfloat16, device=DEV)
        act = torch.full((M, I), float("nan"), dtype=torch.bfloat16, device=DEV)
        hip.call("vlr_gemm_swiglu_lora", x, wgu, gu, act, M, I, K, K, u, 2 * R, Bgu, R)
        return gu, act
    run(f_swiglu, 2)
    # qkv + RoPE: three sub-targets
    nh = nkv = 8
    Nq = Nkv = nh * hd
    Nqkv, rope_cols, max_pos = Nq + 2 * Nkv, Nq + Nkv, 700
    wq, Bq = rnd(Nqkv, K, scale=0.05, seed=8), rnd(Nqkv, R, scale=0.05, seed=9)
    pos = torch.randint(0, max_pos, (M,), generator=g, dtype=torch.int32).to(DEV)
    cos = torch.empty(max_pos, hd // 2, dtype=torch.float32, device=DEV)
    sin = torch.empty_like(cos)
    hip.call("vlr_rope_table", cos, sin, max_pos, hd, 10000.0)

    def f_qkv(u):
        out = torch.full((M, Nqkv), float("nan"), dtype=torch.bfloat16, device=DEV)
        hip.call("vlr_gemm_qkv_rope_lora", x, wq, None, out, pos, cos, sin, M, Nqkv, rope_cols, K, K, hd, max_pos, u, 3 * R, Bq, R, Nq, Nkv)
        return (out,)
    run(f_qkv, 3)
    assert hip.helper("vlr_gemm_seg_rowskip", None, 0) == 0


@pytest.mark.parametrize("shape", [(4352, 4352, 512), (12792, 4096, 256), (4104, 4360, 320)])
def test_gemm_residual_continuous(hip, shape):
    """NT GEMM with a residual add at shapes the persistent kernels take (o_proj / down_proj of the forward), out of place and in
    place (C == residual).  The residual epilogue of the continuous pipeline itself (plain GEMMs with a bf16 residual never take it:
    measured slower) is what test_gemm_lora_segment runs with residual=True."""
    M, N, K = shape
    x, W, resid = rnd(M, K, seed=1), rnd(N, K, scale=0.05, seed=2), rnd(M, N, seed=3)
    ref = x.float() @ W.float().t() + resid.float()
    y = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_bf16", 0, x, W, y, None, resid, M, N, K, K, K, N, N, 0, 0, 0)
    torch.cuda.synchronize()
    check(y, ref, 8e-3, f"residual cont {shape}")
    y2 = resid.clone()
    hip.call("vlr_gemm_bf16", 0, x, W, y2, None, y2, M, N, K, K, K, N, N, 0, 0, 0)
    torch.cuda.synchronize()
    check(y2, ref, 8e-3, f"residual in place {shape}")


@pytest.mark.parametrize("shape", [(12792, 4096, 128, 0.05), (4104, 4360, 64, 0.25), (6400, 11008, 24, 0.1), (300, 256, 16, 0.5)])
def test_gemm_dropout_acc(hip, shape):
    """vlr_gemm_dropout_acc: dx += s/(1-p) mask .* (v A) with the mask regenerated in the GEMM epilogue - the kept / dropped
    positions are EXACTLY those of vlr_dropout_mask for the same seed, the values those of the fp32 product."""
    M, n_in, r, pdrop = shape
    seed, scale = 0x1234567 + r, 1.75
    v = rnd(M, 3 * r, scale=0.5, seed=1)[:, r:2 * r]          # one target's slice of the [M][n r] buffer
    A = rnd(r, n_in, scale=0.1, seed=2)
    dx0 = rnd(M, n_in, seed=3)
    mask = torch.empty(M * n_in, dtype=torch.uint8, device=DEV)
    hip.call("vlr_dropout_mask", mask, M * n_in, pdrop, seed)
    keep = mask.view(M, n_in).bool()
    prod = v.float() @ A.float()
    ref = dx0.float() + torch.where(keep, prod * (scale / (1 - pdrop)), torch.zeros_like(prod))
    dx = dx0.clone()
    scratch = torch.empty(M, n_in, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_dropout_acc", v, 3 * r, A, dx, scratch, M, n_in, r, pdrop, seed, scale)
    torch.cuda.synchronize()
    check(dx, ref, 8e-3, f"dropout acc {shape}")
    assert torch.equal(dx[~keep], dx0[~keep])                 # dropped positions are untouched, bit for bit
    assert 0.5 * pdrop < float((~keep).float().mean()) < 1.5 * pdrop


# ---------------------------------------------------------------------------------------------------- grouped-query attention
@pytest.mark.parametrize("B,S,nh,nkv,masked", [(2, 200, 4, 2, True), (1, 333, 8, 2, True), (3, 130, 4, 1, False), (9, 70, 2, 1, False)])
def test_attention_gqa_fwd_bwd(hip, B, S, nh, nkv, masked):
    """vlr_attn_fwd_gqa / vlr_attn_bwd_gqa (Mistral 32/8-style head sharing) against eager attention with repeated K/V heads;
    batch * kv_heads not a multiple of 8 exercises the padding workgroups of the XCD-aware block map."""
    hd = 128
    Hq, Hkv = nh * hd, nkv * hd
    N = Hq + 2 * Hkv
    qkv = rnd(B * S, N, seed=31)
    do = rnd(B * S, Hq, seed=32)
    km = None
    if masked:
        km = torch.ones(B, S, dtype=torch.int32, device=DEV)
        km[0, S - 9:] = 0
        do[S - 9:S] = 0
    scale = 1.0 / math.sqrt(hd)
    Sp = (S + 63) // 64 * 64
    o = torch.full((B * S, Hq), float("nan"), dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(B, nh, Sp, dtype=torch.float32, device=DEV)
    hip.call("vlr_attn_fwd_gqa", qkv, qkv[:, Hq:], qkv[:, Hq + Hkv:], N, o, Hq, lse, km, B, S, nh, nkv, hd, 1, scale)
    dqkv = torch.full((B * S, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    delta = torch.zeros(B, nh, Sp, dtype=torch.float32, device=DEV)
    hip.call("vlr_attn_bwd_gqa", qkv, qkv[:, Hq:], qkv[:, Hq + Hkv:], N, o, do, Hq, lse, delta, km, dqkv, dqkv[:, Hq:],
             dqkv[:, Hq + Hkv:], N, B, S, nh, nkv, hd, 1, scale)
    torch.cuda.synchronize()
    x = qkv.float().requires_grad_(True)
    q = x[:, :Hq].reshape(B, S, nh, hd).transpose(1, 2)
    k = x[:, Hq:Hq + Hkv].reshape(B, S, nkv, hd).transpose(1, 2).repeat_interleave(nh // nkv, dim=1)
    v = x[:, Hq + Hkv:].reshape(B, S, nkv, hd).transpose(1, 2).repeat_interleave(nh // nkv, dim=1)
    ref = ref_attention(q, k, v, True, km, scale).transpose(1, 2).reshape(B * S, Hq)
    (ref * do.float()).sum().backward()
    g = x.grad
    valid = torch.ones(B * S, dtype=torch.bool, device=DEV) if km is None else (km.reshape(-1) != 0)
    check(o[valid], ref[valid], 1.2e-2, "gqa fwd")
    check(dqkv[valid][:, :Hq], g[valid][:, :Hq], 2e-2, "gqa dq")
    check(dqkv[valid][:, Hq:Hq + Hkv], g[valid][:, Hq:Hq + Hkv], 2e-2, "gqa dk")
    check(dqkv[valid][:, Hq + Hkv:], g[valid][:, Hq + Hkv:], 2e-2, "gqa dv")
    assert torch.isfinite(dqkv.float()).all() and torch.isfinite(o.float()).all()


@pytest.mark.parametrize("shape", [(4104, 4352, 512), (4352, 4360, 320), (12792, 1536, 256), (1406, 11008, 4096), (300, 256, 128)])
def test_gemm_swiglu_bwd_fused(hip, shape):
    """vlr_gemm_swiglu_bwd: d act = dy Wdown stays in the accumulators, gate | up are replaced in place by d gate | d up; against the
    fp32 reference and against the unfused pair (plain dgrad GEMM + vlr_swiglu_bwd), incl. a ragged M / I and the small-shape fallback."""
    M, I, H = shape
    assert M < 1000 or ((M + 255) // 256) * ((I + 255) // 256) > 256, "pick shapes the persistent fused kernel takes (> 256 tiles)"
    dy = rnd(M, H, seed=1)
    w = rnd(H, I, scale=0.05, seed=2)
    gu0 = rnd(M, 2 * I, seed=3)
    g, u = gu0[:, :I].float(), gu0[:, I:].float()
    dact = dy.float() @ w.float()
    sg = torch.sigmoid(g)
    ref = torch.cat([dact * u * sg * (1 + g * (1 - sg)), dact * g * sg], dim=1)
    gu = gu0.clone()
    ws = torch.empty(M, I, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_swiglu_bwd", dy, w, gu, ws, M, I, H)
    torch.cuda.synchronize()
    check(gu, ref, 8e-3, f"swiglu bwd fused {shape}")
    gu2 = gu0.clone()
    hip.call("vlr_gemm_bf16", 1, dy, w, ws, None, None, M, I, H, H, I, I, 0, 0, 0, 0)
    hip.call("vlr_swiglu_bwd", gu2, ws, M, I)
    torch.cuda.synchronize()
    check(gu, gu2, 1.6e-2, f"fused vs unfused {shape}")


@pytest.mark.parametrize("shape,average", [((2100, 8200, 512), False), ((2304, 32064, 256), True), ((300, 512, 128), False)])
def test_lmhead_logps_fused(hip, shape, average):
    """vlr_lmhead_logps_fwd / _bwd: fused lm-head + log-softmax pick (no [R][V] logits in HBM when the persistent kernel takes the
    shape; V not a multiple of 256 -> a partial last column tile) against torch log_softmax and against the unfused entry points."""
    R, V, H = shape
    hg = rnd(R, H, seed=1)
    w = rnd(V, H, scale=0.2, seed=2)
    g = torch.Generator().manual_seed(3)
    tgt = torch.randint(0, V, (R,), generator=g, dtype=torch.int32).to(DEV)
    tgt[:4] = torch.tensor([0, V - 1, 255, 256], dtype=torch.int32)          # tile boundaries and the last valid column
    nseq = 5
    cuts = torch.sort(torch.randint(1, R, (nseq - 1,), generator=g)).values.tolist()
    seq_off = torch.tensor([0] + cuts + [R], dtype=torch.int32, device=DEV)
    dlogps = torch.randn(nseq, generator=g).to(DEV)
    fused = bool(hip.helper("vlr_lmhead_is_fused", R, V, H))
    assert fused == (R >= 2000)
    ws = torch.empty(int(hip.lib().vlr_lmhead_workspace_bytes(R, V)), dtype=torch.uint8, device=DEV)
    logits_ws = None if fused else torch.empty(R, V, dtype=torch.float32, device=DEV)
    tok = torch.full((R,), float("nan"), device=DEV)
    lse = torch.full((R,), float("nan"), device=DEV)
    hip.call("vlr_lmhead_logps_fwd", hg, w, tgt, tok, lse, ws, logits_ws, R, V, H)
    dl = torch.full((R, V), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_lmhead_logps_bwd", hg, w, tgt, lse, seq_off, nseq, dlogps, int(average), dl, ws, logits_ws, R, V, H)
    torch.cuda.synchronize()
    logits = hg.float() @ w.float().t()
    ref_lse = torch.logsumexp(logits, -1)
    ref_tok = logits.gather(1, tgt.long()[:, None]).squeeze(1) - ref_lse
    assert float((lse - ref_lse).abs().max()) < 2e-3 and float((tok - ref_tok).abs().max()) < 2e-3
    seq = torch.bucketize(torch.arange(R, device=DEV), seq_off[1:].long(), right=True)
    coef = dlogps[seq]
    if average:
        coef = coef / (seq_off[1:] - seq_off[:-1]).float()[seq]
    ref_dl = coef[:, None] * (torch.nn.functional.one_hot(tgt.long(), V).float() - torch.softmax(logits, -1))
    check(dl, ref_dl, 8e-3, f"lm-head d logits {shape}")
    assert torch.isfinite(dl.float()).all()


# ---------------------------------------------------------------------------------------------------- fp32 residual stream (ABI v4)
@pytest.mark.parametrize("M,H", [(37, 256), (513, 4096)])
def test_rmsnorm_f32_stream(hip, M, H):
    """vlr_rmsnorm_fwd_f32 / _bwd_f32: x is the fp32 residual stream (values that are NOT bf16-representable), y / gradients bf16."""
    x = rnd(M, H, seed=1, dtype=torch.float32) * (1 + 1e-3 * rnd(M, H, seed=7, dtype=torch.float32))
    w, dy, dres = (1 + 0.1 * rnd(H, seed=2).float()).bfloat16(), rnd(M, H, seed=3), rnd(M, H, seed=4)
    y = torch.empty(M, H, dtype=torch.bfloat16, device=DEV)
    rstd = torch.empty(M, dtype=torch.float32, device=DEV)
    hip.call("vlr_rmsnorm_fwd_f32", x, w, y, rstd, M, H, 1e-5)
    xf = x.clone().requires_grad_(True)
    wf = w.float().requires_grad_(True)
    ref = O.rms_norm(xf, wf, 1e-5)
    torch.cuda.synchronize()
    check(y, ref, 5e-3, "rmsnorm fwd f32")
    check(rstd, torch.rsqrt(x.pow(2).mean(-1) + 1e-5), 1e-5, "rstd f32")
    (ref * dy.float()).sum().backward()
    ws = torch.empty(hip.helper("vlr_rmsnorm_bwd_workspace_bytes", H), dtype=torch.uint8, device=DEV)
    dx = torch.empty(M, H, dtype=torch.bfloat16, device=DEV)
    dw = torch.empty(H, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_rmsnorm_bwd_f32", dy, x, w, rstd, dres, dx, dw, 0, ws, M, H)
    torch.cuda.synchronize()
    check(dx, xf.grad + dres.float(), 8e-3, "rmsnorm dx f32")
    check(dw, wf.grad, 8e-3, "rmsnorm dw f32")


# small: 128x128 kernel; (2048, 4096): 128 tiles of 256^2 -> per-tile kernel, fp32 patches; big ones: persistent continuous pipeline
# with the register-direct fp32 epilogue, a peeled tail on the split-K path (12792 rows), ragged N
F32RES_SHAPES = [(300, 264, 136), (2048, 4096, 1024), (12792, 4096, 512), (8200, 4360, 320)]


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("shape", F32RES_SHAPES)
def test_gemm_f32res(hip, shape, inplace):
    """vlr_gemm_bf16_f32res: C fp32 = A B^T + residual fp32 - bf16 x bf16 products are exact in fp32, so the result matches the fp32
    reference to accumulation-order noise (nothing is rounded to bf16)."""
    M, N, K = shape
    a, b = rnd(M, K, seed=1, scale=0.3), rnd(N, K, seed=2, scale=0.3)
    res = rnd(M, N, seed=3, dtype=torch.float32) * 1.001
    ref = a.float() @ b.float().t() + res
    c = res.clone() if inplace else torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    hip.call("vlr_gemm_bf16_f32res", 0, a, b, c, c if inplace else res, M, N, K, K, K, N, N)
    torch.cuda.synchronize()
    check(c, ref, 2e-5, f"gemm f32res {shape} inplace={inplace}")
    if not inplace:                      # no residual
        hip.call("vlr_gemm_bf16_f32res", 0, a, b, c, None, M, N, K, K, K, N, 0)
        torch.cuda.synchronize()
        check(c, a.float() @ b.float().t(), 2e-5, f"gemm f32 out {shape}")


@pytest.mark.parametrize("shape", [(4352, 4352, 512, 128), (12792, 4096, 256, 64), (300, 256, 128, 16)])
def test_gemm_lora_f32res(hip, shape):
    """vlr_gemm_lora_f32res: y fp32 = x W^T + u Bl^T + residual fp32 (adapter segment in the K loop on the big shapes)"""
    M, N, K, r = shape
    x, W = rnd(M, K, seed=1), rnd(N, K, scale=0.05, seed=2)
    ldu = 7 * r
    ubuf = rnd(M, ldu, scale=0.5, seed=3)
    u = ubuf[:, 3 * r:4 * r]
    Bl = rnd(N, r, scale=0.05, seed=4)
    resid = rnd(M, N, seed=5, dtype=torch.float32) * 1.001
    ref = _blockdiag_add(x.float() @ W.float().t(), u, Bl, r, [N]) + resid
    y = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    hip.call("vlr_gemm_lora_f32res", x, K, W, y, N, resid, N, M, N, K, u, ldu, Bl, r)
    torch.cuda.synchronize()
    check(y, ref, 2e-5, f"gemm_lora_f32res {shape}")


def test_decoder_layer_f32_stream(hip):
    """vlr_decoder_layer_fwd / _bwd with vlr_llama_cfg.resid_f32 = 1: the stream enters and leaves in fp32; against the oracle that
    rounds only what this path rounds (MFMA operands), and fp32 autograd for the gradients."""
    from vlrlhf import _hip as HH
    B, S, nh, hd, I = 2, 70, 2, 128, 384
    H = nh * hd
    M = B * S
    cfgo = dict(hidden=H, inter=I, layers=1, heads=nh, vocab=8, rms_eps=1e-5)
    g = torch.Generator().manual_seed(0)
    W = {}
    p = "language_model.model.layers.0."
    for nm, shp in (("self_attn.q_proj", (H, H)), ("self_attn.k_proj", (H, H)), ("self_attn.v_proj", (H, H)),
                    ("self_attn.o_proj", (H, H)), ("mlp.gate_proj", (I, H)), ("mlp.up_proj", (I, H)), ("mlp.down_proj", (H, I))):
        W[p + nm + ".weight"] = (torch.randn(*shp, generator=g) * 0.05).bfloat16().float()
    W[p + "input_layernorm.weight"] = (1 + 0.1 * torch.randn(H, generator=g)).bfloat16().float()
    W[p + "post_attention_layernorm.weight"] = (1 + 0.1 * torch.randn(H, generator=g)).bfloat16().float()
    W["language_model.model.norm.weight"] = torch.ones(H)
    x = torch.randn(B, S, H, generator=g)                       # fp32 stream: not bf16-representable
    am = torch.ones(B, S, dtype=torch.long)
    am[1, S - 6:] = 0
    pos = (am.cumsum(-1) - 1).masked_fill(am == 0, 1)
    dy = torch.randn(B, S, H, generator=g).bfloat16().float()
    dy[am == 0] = 0
    leaves = {k: v.clone().requires_grad_(True) for k, v in W.items()}
    xg = x.clone().requires_grad_(True)
    col = []
    O.llama_hidden(xg, am, pos, leaves, cfgo, emulate_bf16=False, collect=col)
    (col[0] * dy).sum().backward()
    col16 = []
    with torch.no_grad():
        O.llama_hidden(x, am, pos, W, cfgo, emulate_bf16=frozenset(("w", "xn", "rope", "v", "p", "attn", "act", "hidden")), collect=col16)

    def dv(t, dt=torch.bfloat16):
        return t.to(dt).to(DEV).contiguous()

    wqkv = dv(torch.cat([W[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], 0))
    wgu = dv(torch.cat([W[p + "mlp.gate_proj.weight"], W[p + "mlp.up_proj.weight"]], 0))
    wo, wdown = dv(W[p + "self_attn.o_proj.weight"]), dv(W[p + "mlp.down_proj.weight"])
    ln1, ln2 = dv(W[p + "input_layernorm.weight"]), dv(W[p + "post_attention_layernorm.weight"])
    cos_t = torch.empty(256, hd // 2, device=DEV)
    sin_t = torch.empty_like(cos_t)
    hip.call("vlr_rope_table", cos_t, sin_t, 256, hd, 10000.0)
    cfg = HH.LlamaCfg(H, I, nh, hd, 1e-5, 256, cos_t.data_ptr(), sin_t.data_ptr(), 0, 1)
    lw = HH.LayerWeights(*(t.data_ptr() for t in (ln1, wqkv, wo, ln2, wgu, wdown)))
    Sp = (S + 63) // 64 * 64
    f32 = ("rstd1", "rstd2", "lse", "x_mid", "x_out")
    shapes = dict(xn1=(M, H), rstd1=(M,), qkv=(M, 3 * H), attn=(M, H), lse=(B, nh, Sp), x_mid=(M, H), xn2=(M, H), rstd2=(M,), gu=(M, 2 * I),
                  act=(M, I), x_out=(M, H))
    bufs = {k: torch.zeros(*s, dtype=torch.float32 if k in f32 else torch.bfloat16, device=DEV) for k, s in shapes.items()}
    la = HH.LayerActs(*(bufs[k].data_ptr() for k in ("xn1", "rstd1", "qkv", "attn", "lse", "x_mid", "xn2", "rstd2", "gu", "act", "x_out")))
    xin = dv(x.reshape(M, H), torch.float32)
    posd = pos.to(torch.int32).to(DEV)
    kmd = am.to(torch.int32).to(DEV)
    hip.call("vlr_decoder_layer_fwd", cfg, lw, la, xin, posd, kmd, B, S)
    torch.cuda.synchronize()
    valid = (am.reshape(-1) != 0)
    e_emu = relerr(bufs["x_out"].cpu()[valid], col16[0].reshape(M, H)[valid])
    e_f32 = relerr(bufs["x_out"].cpu()[valid], col[0].detach().reshape(M, H)[valid])
    assert e_emu < 4e-3 and e_f32 < 6e-3, (e_emu, e_f32)       # the bf16 stream sits at 1-2e-2 here (test_decoder_layer_fwd_bwd_vs_oracle)
    grads = {k: torch.full_like(t, float("nan")) for k, t in dict(ln1=ln1, wqkv=wqkv, wo=wo, ln2=ln2, wgu=wgu, wdown=wdown).items()}
    lg = HH.LayerGrads(*(grads[k].data_ptr() for k in ("ln1", "wqkv", "wo", "ln2", "wgu", "wdown")))
    wsb = {k: torch.empty(*s, dtype=torch.bfloat16, device=DEV) for k, s in dict(dact=(M, I), dxn=(M, H), dattn=(M, H), dqkv=(M, 3 * H), dx_mid=(M, H)).items()}
    delta = torch.zeros(B, nh, Sp, dtype=torch.float32, device=DEV)
    nws = torch.empty(hip.helper("vlr_rmsnorm_bwd_workspace_bytes", H), dtype=torch.uint8, device=DEV)
    lws = HH.LayerBwdWs(wsb["dact"].data_ptr(), wsb["dxn"].data_ptr(), wsb["dattn"].data_ptr(), wsb["dqkv"].data_ptr(),
                        wsb["dx_mid"].data_ptr(), delta.data_ptr(), nws.data_ptr())
    dxin = torch.empty(M, H, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_decoder_layer_bwd", cfg, lw, lg, 0, la, lws, xin, dv(dy.reshape(M, H)), dxin, posd, kmd, B, S)
    torch.cuda.synchronize()
    check(dxin.cpu()[valid], xg.grad.reshape(M, H)[valid], 4e-2, "layer dx (f32 stream)")
    gq = torch.cat([leaves[p + f"self_attn.{n}_proj.weight"].grad for n in "qkv"], 0)
    check(grads["wqkv"].cpu(), gq, 4e-2, "dWqkv (f32 stream)")
    check(grads["wdown"].cpu(), leaves[p + "mlp.down_proj.weight"].grad, 4e-2, "dWdown (f32 stream)")
    check(grads["ln2"].cpu(), leaves[p + "post_attention_layernorm.weight"].grad, 4e-2, "dln2 (f32 stream)")


# ---------------------------------------------------------------------------------------------------- attention at the sizes the step runs
@pytest.mark.parametrize("B,S,nh,nkv", [(2, 1599, 32, 32), (1, 4975, 32, 8)])
def test_attention_at_step_sizes(hip, B, S, nh, nkv):
    """Kernel-level parity at the sequence lengths and head counts of the benchmark configurations: S = 1599 with 32 heads (BASELINE
    configs[1]) and S = 4975 with 32 query / 8 K/V heads (configs[3], LLaVA-Next-Mistral) - forward AND backward against an fp32 eager
    reference evaluated one query head at a time (S x S fp32 per head), with right padding on the first sequence."""
    hd = 128
    Hq, Hkv = nh * hd, nkv * hd
    N = Hq + 2 * Hkv
    grp = nh // nkv
    qkv = rnd(B * S, N, seed=41)
    do = rnd(B * S, Hq, seed=42)
    km = torch.ones(B, S, dtype=torch.int32, device=DEV)
    km[0, S - 37:] = 0
    do.view(B, S, Hq)[0, S - 37:] = 0
    scale = 1.0 / math.sqrt(hd)
    Sp = (S + 63) // 64 * 64
    o = torch.full((B * S, Hq), float("nan"), dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(B, nh, Sp, dtype=torch.float32, device=DEV)
    hip.call("vlr_attn_fwd_gqa", qkv, qkv[:, Hq:], qkv[:, Hq + Hkv:], N, o, Hq, lse, km, B, S, nh, nkv, hd, 1, scale)
    dqkv = torch.full((B * S, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    delta = torch.full((B, nh, Sp), float("nan"), dtype=torch.float32, device=DEV)
    hip.call("vlr_attn_bwd_gqa", qkv, qkv[:, Hq:], qkv[:, Hq + Hkv:], N, o, do, Hq, lse, delta, km, dqkv, dqkv[:, Hq:],
             dqkv[:, Hq + Hkv:], N, B, S, nh, nkv, hd, 1, scale)
    torch.cuda.synchronize()
    ref = torch.empty(B * S, Hq, device=DEV)
    g = torch.zeros(B * S, N, device=DEV)
    tril = torch.ones(S, S, dtype=torch.bool, device=DEV).tril()
    for b in range(B):
        rows = slice(b * S, (b + 1) * S)
        vis = tril & (km[b][None, :] != 0)
        for h in range(nh):
            kv = h // grp
            q = qkv[rows, h * hd:(h + 1) * hd].float().requires_grad_(True)
            k = qkv[rows, Hq + kv * hd: Hq + (kv + 1) * hd].float().requires_grad_(True)
            v = qkv[rows, Hq + Hkv + kv * hd: Hq + Hkv + (kv + 1) * hd].float().requires_grad_(True)
            p = torch.softmax(((q @ k.t()) * scale).masked_fill(~vis, float("-inf")), -1)
            r = p @ v
            (r * do[rows, h * hd:(h + 1) * hd].float()).sum().backward()
            ref[rows, h * hd:(h + 1) * hd] = r.detach()
            g[rows, h * hd:(h + 1) * hd] = q.grad
            g[rows, Hq + kv * hd: Hq + (kv + 1) * hd] += k.grad              # K/V heads are shared by `grp` query heads
            g[rows, Hq + Hkv + kv * hd: Hq + Hkv + (kv + 1) * hd] += v.grad
            del q, k, v, p, r
    valid = km.reshape(-1) != 0
    check(o[valid], ref[valid], 1.2e-2, f"attention fwd S={S}")
    check(dqkv[valid][:, :Hq], g[valid][:, :Hq], 2e-2, f"dq S={S}")
    check(dqkv[valid][:, Hq:Hq + Hkv], g[valid][:, Hq:Hq + Hkv], 2e-2, f"dk S={S}")
    check(dqkv[valid][:, Hq + Hkv:], g[valid][:, Hq + Hkv:], 2e-2, f"dv S={S}")
    assert torch.isfinite(dqkv.float()).all() and torch.isfinite(o.float()).all()
    assert float(dqkv[~valid][:, Hq:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------- persistent tile schedules
def _with_sched(hip, mode, fn):
    from vlrlhf import _hip as HH
    HH.ensure_splitk_workspace(DEV, force=True)
    assert hip.helper("vlr_gemm_set_sched", mode) == 0
    try:
        return fn()
    finally:
        hip.helper("vlr_gemm_set_sched", -1)


# tiles % 256 != 0 in every case, K >= 1024; (M, N, K): 800 / 688+ / 1376-tile shapes of the 7B step, scaled K
SCHED_SHAPES = [(12792, 4096, 1024), (4096, 11008, 1088), (5000, 4360, 2048)]


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("shape", SCHED_SHAPES)
def test_gemm_sched_modes(hip, layout, shape):
    """vlr_gemm_set_sched: the serial epilogue order (16: the two wave groups one after the other, as before round 4) and the tile maps
    (32: the shared-panel map of gemm_tilemap.h, the default since round 5; without it the per-XCD contiguous ranges of rounds 1-4) - the
    same arithmetic per output tile in another order of the tiles, so bit-identical; each mode twice, and a NaN-filled output proves
    every tile is written.  The removed tile schedules (1-7) are rejected."""
    M, N, K = shape
    if layout == 2:
        K = K + 40
    a, b = rnd(M, K, seed=1, scale=0.5), rnd(N, K, seed=2, scale=0.5)
    ref = a.float() @ b.float().t()
    A = a if layout != 2 else a.t().contiguous()
    Bm = b if layout == 0 else b.t().contiguous()
    lda = K if layout != 2 else M
    ldb = K if layout == 0 else N
    outs = {}
    for mode in (0, 16, 32, 48):
        def run():
            res = []
            for _ in range(2):
                c = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
                hip.call("vlr_gemm_bf16", layout, A, Bm, c, None, None, M, N, K, lda, ldb, N, 0, 0, 0, 0)
                torch.cuda.synchronize()
                res.append(c)
            return res
        c1, c2 = _with_sched(hip, mode, run)
        assert torch.equal(c1, c2), f"mode {mode}: not reproducible"
        check(c1, ref, 8e-3, f"gemm sched {mode} layout {layout} {shape}")
        outs[mode] = c1
    assert torch.equal(outs[0], outs[16]) and torch.equal(outs[0], outs[32]) and torch.equal(outs[0], outs[48])
    for mode in (1, 2, 3, 4, 7, 64):
        assert hip.helper("vlr_gemm_set_sched", mode) != 0
    assert hip.helper("vlr_gemm_set_sched", -1) == 0


def test_gemm_sched_fused_epilogues(hip):
    """the fused SwiGLU / RoPE-free / SwiGLU-backward / fp32-residual launches with the serial epilogue order and with either tile map:
    bit-identical"""
    M, I, H = 6648, 2176, 1024                                   # 26 x 17 = 442 SwiGLU tiles; 26 x 9 o_proj-like tiles
    x, wgu = rnd(M, H, seed=1), rnd(2 * I, H, scale=0.05, seed=2)
    dy, wdown = rnd(M, H, seed=3), rnd(H, I, scale=0.05, seed=4)
    res = rnd(M, 4352, seed=5, dtype=torch.float32)
    wo = rnd(4352, H, scale=0.05, seed=6)
    base = {}
    for mode in (0, 16, 32):
        def run():
            gu = torch.full((M, 2 * I), float("nan"), dtype=torch.bfloat16, device=DEV)
            act = torch.full((M, I), float("nan"), dtype=torch.bfloat16, device=DEV)
            hip.call("vlr_gemm_swiglu", x, wgu, gu, act, M, I, H, H, 1)
            gub = gu.clone()
            dws = torch.empty(M, I, dtype=torch.bfloat16, device=DEV)
            hip.call("vlr_gemm_swiglu_bwd", dy, wdown, gub, dws, M, I, H)
            y = torch.full((M, 4352), float("nan"), dtype=torch.float32, device=DEV)
            hip.call("vlr_gemm_bf16_f32res", 0, x, wo, y, res, M, 4352, H, H, H, 4352, 4352)
            torch.cuda.synchronize()
            return gu, act, gub, y
        out = _with_sched(hip, mode, run)
        assert all(torch.isfinite(t.float()).all() for t in out), mode
        if mode == 0:
            base = out
            g, u = (x.float() @ wgu.float().t()).split(I, dim=1)
            check(out[1], F.silu(g) * u, 8e-3, "swiglu act")
            check(out[3], x.float() @ wo.float().t() + res, 2e-5, "f32res")
        else:
            for t0, t1 in zip(base, out):
                assert torch.equal(t0, t1), f"fused epilogue under sched {mode}"


@pytest.mark.parametrize("shape", [((22016, 4096), (4096, 11008), 1064),      # the dW_gate|up + dW_down pair of the 7B layer: one tile row peeled
                                   ((4096, 4096), (4096, 11008), 520),       # 256 + 688 tiles: no peel
                                   ((2048, 1024), (1024, 2816), 300)])       # 32 + 44 tiles: fewer than the CUs -> two plain calls
def test_gemm_tn_pair(hip, shape):
    """vlr_gemm_bf16_tn_pair: two weight-gradient GEMMs as one persistent launch - against fp32 torch, and bit-identical to two
    vlr_gemm_bf16 calls on every row the 256x256 kernel computes in both (the peeled tile row runs split along K: tolerance only);
    NaN-filled outputs prove every element is written; accumulate = 1 takes the two-call path and adds."""
    (M0, N0), (M1, N1), K = shape
    a0, b0 = rnd(K, M0, seed=1, scale=0.5), rnd(K, N0, seed=2, scale=0.5)
    a1, b1 = rnd(K, M1, seed=3, scale=0.5), rnd(K, N1, seed=4, scale=0.5)
    c0 = torch.full((M0, N0), float("nan"), dtype=torch.bfloat16, device=DEV)
    c1 = torch.full((M1, N1), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_bf16_tn_pair", a0, b0, c0, M0, N0, M0, N0, N0, a1, b1, c1, M1, N1, M1, N1, N1, K, 0)
    torch.cuda.synchronize()
    r0, r1 = a0.float().t() @ b0.float(), a1.float().t() @ b1.float()
    check(c0, r0, 8e-3, f"tn pair, problem 0 {shape}")
    check(c1, r1, 8e-3, f"tn pair, problem 1 {shape}")
    s0, s1 = torch.empty_like(c0), torch.empty_like(c1)
    hip.call("vlr_gemm_bf16", 2, a0, b0, s0, None, None, M0, N0, K, M0, N0, N0, 0, 0, 0, 0)
    hip.call("vlr_gemm_bf16", 2, a1, b1, s1, None, None, M1, N1, K, M1, N1, N1, 0, 0, 0, 0)
    torch.cuda.synchronize()
    # rows that the 256x256 kernel computes in the separate launches AND in the pair (the separate launches peel nothing at these shapes
    # or other rows): identical K order -> identical bits on the overwhelming majority of rows; everything within the GEMM tolerance
    same0 = (c0 == s0).all(dim=1).float().mean().item()
    same1 = (c1 == s1).all(dim=1).float().mean().item()
    assert same0 > 0.9 and same1 > 0.9, (same0, same1)
    check(c0, s0, 8e-3, "pair vs single, problem 0")
    check(c1, s1, 8e-3, "pair vs single, problem 1")
    c0b, c1b = c0.clone(), c1.clone()
    hip.call("vlr_gemm_bf16_tn_pair", a0, b0, c0b, M0, N0, M0, N0, N0, a1, b1, c1b, M1, N1, M1, N1, N1, K, 1)
    torch.cuda.synchronize()
    check(c0b, 2 * r0, 1.2e-2, "tn pair accumulate 0")
    check(c1b, 2 * r1, 1.2e-2, "tn pair accumulate 1")


# ---------------------------------------------------------------------------------------------------- grouped skinny GEMMs (LoRA)
@pytest.mark.parametrize("M,in_,r,groups", [(12792, 4096, 128, 3), (1406, 1024, 64, 2), (300, 256, 16, 1)])
def test_gemm_grouped_masked(hip, M, in_, r, groups):
    """vlr_gemm_grouped: (a) u_t = alpha * (mask_t . x) A_t^T for the targets of a LoRA group in one launch, the keep mask of
    vlr_dropout(seed + t) applied to x while it is staged (NT, mask_on 1); (b) dA_t = alpha * v_t^T (mask_t . x) (TN, mask_on 2, split
    along K = tokens); (c) v_t = dy_t B_t (NN, grouped column blocks) - against torch with the masks of vlr_dropout_mask."""
    from vlrlhf import _hip as HH
    HH.ensure_splitk_workspace(DEV, force=True)
    p, seed, alpha = 0.25, 1234567, 2.0 / 0.75
    x = rnd(M, in_, seed=1)
    A = rnd(groups * r, in_, seed=2, scale=0.05)
    masks = []
    for t in range(groups):
        mk = torch.empty(M * in_, dtype=torch.uint8, device=DEV)
        hip.call("vlr_dropout_mask", mk, M * in_, p, seed + t)
        masks.append(mk.view(M, in_).float())
    # (a)
    ldu = 7 * r
    u = torch.full((M, ldu), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_grouped", 0, x, A, u, M, r, in_, in_, in_, ldu, groups, 0, r * in_, r, alpha, 0, 1, seed, p, in_)
    torch.cuda.synchronize()
    for t in range(groups):
        ref = alpha * (x.float() * masks[t]) @ A[t * r:(t + 1) * r].float().t()
        check(u[:, t * r:(t + 1) * r], ref, 8e-3, f"grouped masked NT, target {t}")
    assert torch.isnan(u[:, groups * r:].float()).all()
    # (b)
    v = rnd(M, groups * r, seed=3, scale=0.5)
    dA = torch.full((groups * r, in_), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_grouped", 2, v, x, dA, r, in_, M, groups * r, in_, in_, groups, r, 0, r * in_, alpha, 0, 2, seed, p, in_)
    torch.cuda.synchronize()
    for t in range(groups):
        ref = alpha * v[:, t * r:(t + 1) * r].float().t() @ (x.float() * masks[t])
        check(dA[t * r:(t + 1) * r], ref, 8e-3, f"grouped masked TN, target {t}")
    # (c) + accumulate
    out = 256
    dy = rnd(M, groups * out, seed=4)
    Bw = rnd(groups * out, r, seed=5, scale=0.05)
    vv = torch.ones(M, groups * r, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_grouped", 1, dy, Bw, vv, M, r, out, groups * out, r, groups * r, groups, out, out * r, r, 1.0, 1, 0, 0, 0.0, 0)
    torch.cuda.synchronize()
    for t in range(groups):
        ref = 1.0 + dy[:, t * out:(t + 1) * out].float() @ Bw[t * out:(t + 1) * out].float()
        check(vv[:, t * r:(t + 1) * r], ref, 8e-3, f"grouped NN accumulate, target {t}")


@pytest.mark.parametrize("M,in_,r,n,p", [(12792, 4096, 128, 3, 0.05), (1406, 1024, 64, 2, 0.25), (300, 256, 16, 1, 0.0), (2248, 2048, 256, 2, 0.05), (1000, 1024, 256, 1, 0.0)])
def test_gemm_dropout_acc_multi(hip, M, in_, r, n, p):
    """vlr_gemm_dropout_acc_multi: dx (+)= scale / (1 - p) * sum_t mask_t . (v_t A_t) for the n targets of a group in ONE pass over dx,
    against torch with the masks of vlr_dropout_mask; both the accumulate and the write form"""
    seed, scale = 4242, 2.0
    v = rnd(M, n * r, seed=1, scale=0.5)
    A = rnd(n * r, in_, seed=2, scale=0.05)
    dx0 = rnd(M, in_, seed=3)
    ref = torch.zeros(M, in_, device=DEV)
    for t in range(n):
        if p > 0:
            mk = torch.empty(M * in_, dtype=torch.uint8, device=DEV)
            hip.call("vlr_dropout_mask", mk, M * in_, p, seed + t)
            mk = mk.view(M, in_).float()
        else:
            mk = 1.0
        ref += scale / (1 - p) * mk * (v[:, t * r:(t + 1) * r].float() @ A[t * r:(t + 1) * r].float())
    dx = dx0.clone()
    hip.call("vlr_gemm_dropout_acc_multi", n, v, n * r, A, dx, M, in_, r, p, seed, scale, 1)
    torch.cuda.synchronize()
    check(dx, dx0.float() + ref, 8e-3, "dropacc multi (accumulate)")
    dx = torch.full((M, in_), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_dropout_acc_multi", n, v, n * r, A, dx, M, in_, r, p, seed, scale, 0)
    torch.cuda.synchronize()
    check(dx, ref, 8e-3, "dropacc multi (write)")


@pytest.mark.parametrize("shape", [(4104, 4352, 512), (300, 256, 128)])
def test_gemm_swiglu_bwd_add(hip, shape):
    """vlr_gemm_swiglu_bwd_add: d act = dy Wdown + addend before the SwiGLU backward (the addend buffer is also the fallback scratch)"""
    M, I, H = shape
    dy = rnd(M, H, seed=1)
    w = rnd(H, I, scale=0.05, seed=2)
    gu0 = rnd(M, 2 * I, seed=3)
    add = rnd(M, I, seed=4, scale=0.3)
    g, u = gu0[:, :I].float(), gu0[:, I:].float()
    dact = dy.float() @ w.float() + add.float()
    sg = torch.sigmoid(g)
    ref = torch.cat([dact * u * sg * (1 + g * (1 - sg)), dact * g * sg], dim=1)
    gu = gu0.clone()
    ws = add.clone()
    hip.call("vlr_gemm_swiglu_bwd_add", dy, w, gu, ws, ws, M, I, H)
    torch.cuda.synchronize()
    check(gu, ref, 1.6e-2, f"swiglu bwd + addend {shape}")


# ---------------------------------------------------------------------------------------------------- CUs left to RCCL
@pytest.mark.parametrize("k", [16, 40])
def test_persistent_kernels_with_comm_cus(hip, k):
    """vlr_set_comm_cus(k): the persistent GEMM (plain, fused SwiGLU, fp32-residual) and attention-forward launches run on (CUs - k) rounded
    to whole XCD octets - same results as on the full chip up to summation order (the peel and the persistent grid change)"""
    assert hip.helper("vlr_set_comm_cus", k) == 0
    try:
        assert hip.helper("vlr_compute_cus") == 256 - (k + 7) // 8 * 8
        M, N, K = 12792, 4096, 1024
        a, b = rnd(M, K, seed=1, scale=0.5), rnd(N, K, seed=2, scale=0.5)
        c = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        hip.call("vlr_gemm_bf16", 0, a, b, c, None, None, M, N, K, K, K, N, 0, 0, 0, 0)
        res = rnd(M, N, seed=3, dtype=torch.float32)
        cf = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
        hip.call("vlr_gemm_bf16_f32res", 0, a, b, cf, res, M, N, K, K, K, N, N)
        I = 2176
        wgu = rnd(2 * I, K, scale=0.05, seed=4)
        gu = torch.full((M, 2 * I), float("nan"), dtype=torch.bfloat16, device=DEV)
        act = torch.full((M, I), float("nan"), dtype=torch.bfloat16, device=DEV)
        hip.call("vlr_gemm_swiglu", a, wgu, gu, act, M, I, K, K, 1)
        B, S, nh, hd = 8, 1599, 32, 128
        H = nh * hd
        qkv = rnd(B * S, 3 * H, seed=5)
        o = torch.full((B * S, H), float("nan"), dtype=torch.bfloat16, device=DEV)
        lse = torch.zeros(B, nh, (S + 63) // 64 * 64, dtype=torch.float32, device=DEV)
        hip.call("vlr_attn_fwd", qkv, qkv[:, H:], qkv[:, 2 * H:], 3 * H, o, H, lse, None, B, S, nh, hd, 1, 1 / math.sqrt(hd))
        # the backward's launches in the bucket window: a data-gradient GEMM (NN; at 240 CUs 5 tile rows go to the 128x128 kernel: 45 x 16 tiles
        # = 3 rounds) and the weight-gradient pair dW_qkv + dW_o (TN; 4 + 2 rounds apart, 4 + 4 peeled tile rows together)
        bn = rnd(K, N, seed=6, scale=0.5)
        cn = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        hip.call("vlr_gemm_bf16", 1, a, bn, cn, None, None, M, N, K, K, N, N, 0, 0, 0, 0)
        dy, xn, dm, at = rnd(K, 3 * N, seed=7, scale=0.5), rnd(K, N, seed=8, scale=0.5), rnd(K, N, seed=9, scale=0.5), rnd(K, N, seed=10, scale=0.5)
        w0 = torch.full((3 * N, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        w1 = torch.full((N, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        hip.call("vlr_gemm_bf16_tn_pair", dy, xn, w0, 3 * N, N, 3 * N, N, N, dm, at, w1, N, N, N, N, N, K, 0)
        torch.cuda.synchronize()
        check(cn, a.float() @ bn.float(), 8e-3, "NN gemm on a reduced grid")
        check(w0, dy.float().t() @ xn.float(), 8e-3, "TN pair, first problem, on a reduced grid")
        check(w1, dm.float().t() @ at.float(), 8e-3, "TN pair, second problem, on a reduced grid")
        ref = a.float() @ b.float().t()
        check(c, ref, 8e-3, "gemm on a reduced grid")
        check(cf, ref + res, 2e-5, "f32res gemm on a reduced grid")
        g, u = (a.float() @ wgu.float().t()).split(I, dim=1)
        check(act, F.silu(g) * u, 8e-3, "fused swiglu on a reduced grid")
        q, kk, v = (qkv[:S, i * H:i * H + hd].float() for i in range(3))         # sequence 0, head 0
        p = torch.softmax((q @ kk.t() / math.sqrt(hd)).masked_fill(~torch.ones(S, S, dtype=torch.bool, device=DEV).tril(), float("-inf")), -1)
        check(o[:S, :hd], p @ v, 1.2e-2, "attention forward on a reduced grid")
        assert torch.isfinite(o.float()).all()
    finally:
        hip.helper("vlr_set_comm_cus", -1)


# ---------------------------------------------------------------------------------------------------- packed lora_dropout masks (ABI v5)
@pytest.mark.parametrize("M,in_,r,n,p", [(1406, 1024, 64, 3, 0.25), (12792, 4096, 128, 2, 0.05)])
def test_dropout_bits_and_masked_gemms_with_bits(hip, M, in_, r, n, p):
    """vlr_dropout_bits packs exactly the keep mask of vlr_dropout_mask (bit e of byte i = element 8 i + e), and the three adapter kernels
    that take the packed masks (staged NT operand, staged TN operand, dropout-accumulate epilogue: one pass per target and the one-pass
    form) return BIT-IDENTICAL results to the same calls hashing in the kernel."""
    from vlrlhf import _hip as HH
    HH.ensure_splitk_workspace(DEV, force=True)
    seed, alpha, scale = 99, 2.0 / (1 - p), 2.0
    gstride = M * in_ // 8
    bits = torch.zeros(n * gstride, dtype=torch.uint8, device=DEV)
    for t in range(n):
        hip.call("vlr_dropout_bits", bits[t * gstride:], M * in_, p, seed + t)
        mk = torch.empty(M * in_, dtype=torch.uint8, device=DEV)
        hip.call("vlr_dropout_mask", mk, M * in_, p, seed + t)
        torch.cuda.synchronize()
        b = bits[t * gstride:(t + 1) * gstride]
        unpacked = ((b.view(-1, 1) >> torch.arange(8, device=DEV, dtype=torch.uint8)) & 1).reshape(-1)
        assert torch.equal(unpacked, mk), f"packed mask of target {t}"
    x = rnd(M, in_, seed=1)
    A = rnd(n * r, in_, seed=2, scale=0.05)
    ldu = n * r
    u0, u1 = torch.zeros(M, ldu, dtype=torch.bfloat16, device=DEV), torch.zeros(M, ldu, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_grouped", 0, x, A, u0, M, r, in_, in_, in_, ldu, n, 0, r * in_, r, alpha, 0, 1, seed, p, in_)
    hip.call("vlr_gemm_grouped_bits", 0, x, A, u1, M, r, in_, in_, in_, ldu, n, 0, r * in_, r, alpha, 0, 1, seed, p, in_, bits, gstride)
    torch.cuda.synchronize()
    # (the packed-mask form runs on the LDS-DMA ring kernel, the hashing form on the register-staged one: same mask, another summation order)
    for t in range(n):
        mk = ((bits[t * gstride:(t + 1) * gstride].view(-1, 1) >> torch.arange(8, device=DEV, dtype=torch.uint8)) & 1).reshape(M, in_).float()
        ref = alpha * (x.float() * mk) @ A[t * r:(t + 1) * r].float().t()
        check(u1[:, t * r:(t + 1) * r], ref, 8e-3, f"masked NT with packed masks, target {t}")
        check(u0[:, t * r:(t + 1) * r], ref, 8e-3, f"masked NT hashing, target {t}")
    assert float((u0.float() - u1.float()).abs().max()) <= 0.02 * float(u0.float().abs().max())
    v = rnd(M, n * r, seed=3, scale=0.5)
    d0, d1 = torch.zeros(n * r, in_, dtype=torch.bfloat16, device=DEV), torch.zeros(n * r, in_, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_grouped", 2, v, x, d0, r, in_, M, n * r, in_, in_, n, r, 0, r * in_, alpha, 0, 2, seed, p, in_)
    hip.call("vlr_gemm_grouped_bits", 2, v, x, d1, r, in_, M, n * r, in_, in_, n, r, 0, r * in_, alpha, 0, 2, seed, p, in_, bits, gstride)
    torch.cuda.synchronize()
    assert torch.equal(d0, d1), "masked TN (dA = v^T drop(x))"
    # the K-tile-blocked transposed masks (vlr_dropout_bits2) and the TN product that reads them on the LDS-DMA ring kernel (mask_on 3)
    tstride = HH.helper("vlr_dropout_bits_kt_bytes", M, in_)
    bits_rm = torch.zeros(n * gstride, dtype=torch.uint8, device=DEV)
    bits_kt = torch.zeros(n * tstride, dtype=torch.uint8, device=DEV)
    for t in range(n):
        hip.call("vlr_dropout_bits2", bits_rm[t * gstride:], bits_kt[t * tstride:], M, in_, p, seed + t)
    torch.cuda.synchronize()
    assert torch.equal(bits_rm, bits), "row-major half of vlr_dropout_bits2"
    Mp = (M + 63) // 64 * 64
    for t in range(n):
        mk = ((bits[t * gstride:(t + 1) * gstride].view(-1, 1) >> torch.arange(8, device=DEV, dtype=torch.uint8)) & 1).reshape(M, in_)
        mkp = torch.zeros(Mp, in_, dtype=torch.uint8, device=DEV)
        mkp[:M] = mk
        # expected transposed form: [row / 64][col][(row % 64) / 8] bytes, bit = row % 8
        w = (mkp.view(Mp // 64, 8, 8, in_).permute(0, 3, 1, 2).to(torch.int32) << torch.arange(8, device=DEV, dtype=torch.int32)).sum(-1).to(torch.uint8)
        assert torch.equal(bits_kt[t * tstride:(t + 1) * tstride], w.reshape(-1)), f"transposed masks of target {t}"
    d2 = torch.zeros(n * r, in_, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_grouped_bits", 2, v, x, d2, r, in_, M, n * r, in_, in_, n, r, 0, r * in_, alpha, 0, 3, seed, p, in_, bits_kt, tstride)
    torch.cuda.synchronize()
    for t in range(n):
        mk = ((bits[t * gstride:(t + 1) * gstride].view(-1, 1) >> torch.arange(8, device=DEV, dtype=torch.uint8)) & 1).reshape(M, in_).float()
        ref = alpha * v[:, t * r:(t + 1) * r].float().t() @ (x.float() * mk)
        check(d2[t * r:(t + 1) * r], ref, 8e-3, f"masked TN with transposed packed masks, target {t}")
    dx0 = rnd(M, in_, seed=4)
    a0, a1, a2 = dx0.clone(), dx0.clone(), dx0.clone()
    scratch = torch.empty(M, in_, dtype=torch.bfloat16, device=DEV)
    for t in range(n):
        hip.call("vlr_gemm_dropout_acc", v[:, t * r:], n * r, A[t * r:], a0, scratch, M, in_, r, p, seed + t, scale)
        hip.call("vlr_gemm_dropout_acc_bits", v[:, t * r:], n * r, A[t * r:], a1, scratch, M, in_, r, p, seed + t, scale, bits[t * gstride:])
    torch.cuda.synchronize()
    assert torch.equal(a0, a1), "dropout-accumulate, one pass per target"
    hip.call("vlr_gemm_dropout_acc_multi", n, v, n * r, A, a2, M, in_, r, p, seed, scale, 1)
    a3 = dx0.clone()
    hip.call("vlr_gemm_dropout_acc_multi_bits", n, v, n * r, A, a3, M, in_, r, p, seed, scale, 1, bits, gstride)
    torch.cuda.synchronize()
    assert torch.equal(a2, a3), "dropout-accumulate, one pass"


# ---------------------------------------------------------------------------------------------------- streaming row-slab adapter products (ABI v9)
@pytest.mark.parametrize("M,in_,r,n,p,rows", [(1406, 1024, 64, 3, 0.25, False), (12792, 4096, 128, 3, 0.05, False), (1353, 1408, 256, 1, 0.05, True),
                                              (700, 128, 128, 2, 0.0, False), (12792, 11008, 128, 1, 0.05, False), (517, 768, 64, 1, 0.0, True)])
def test_lora_rows_u(hip, M, in_, r, n, p, rows):
    """vlr_lora_rows_u: u_t = alpha (keep_t . x) A_t^T for the targets that share x, against fp32 torch with the SAME packed masks; the
    unmarked rows of a row-restricted adapter (PLoRA) come out zero; ragged last slab; u block stride wider than r (the two-adapter layout);
    the kernel is deterministic (bit-identical twice)."""
    seed, alpha = 77, (2.0 / (1 - p) if p > 0 else 2.0)
    gstride = M * in_ // 8
    bits = None
    if p > 0:
        bits = torch.zeros(n * gstride, dtype=torch.uint8, device=DEV)
        for t in range(n):
            hip.call("vlr_dropout_bits", bits[t * gstride:], M * in_, p, seed + t)
    x = rnd(M, in_, seed=1)
    A = rnd(n * r, in_, seed=2, scale=0.05)
    ustride, ldu = r + 64, n * (r + 64) + 8
    rowmask = None
    if rows:
        g = torch.Generator().manual_seed(5)
        rm = (torch.rand(M, generator=g) < 0.4)
        rm[64:256] = False                       # whole slabs without a marked row
        rowmask = rm.to(torch.uint8).to(DEV)
    outs = []
    for _ in range(2):
        u = torch.full((M, ldu), float("nan"), dtype=torch.bfloat16, device=DEV)
        hip.call("vlr_lora_rows_u", n, x, in_, A, u, ldu, ustride, M, in_, r, alpha, bits, gstride, rowmask)
        torch.cuda.synchronize()
        outs.append(u)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "not deterministic"
    u = outs[0]
    for t in range(n):
        xm = x.float()
        if p > 0:
            mk = ((bits[t * gstride:(t + 1) * gstride].view(-1, 1) >> torch.arange(8, device=DEV, dtype=torch.uint8)) & 1).reshape(M, in_).float()
            xm = xm * mk
        ref = alpha * xm @ A[t * r:(t + 1) * r].float().t()
        if rows:
            ref = ref * rowmask.float().view(-1, 1)
            assert float(u[:, t * ustride:t * ustride + r][~rowmask.bool()].float().abs().max()) == 0.0
        check(u[:, t * ustride:t * ustride + r], ref, 8e-3, f"u of target {t}")
        assert torch.isnan(u[:, t * ustride + r:(t + 1) * ustride].float()).all(), "wrote outside its block"


@pytest.mark.parametrize("M,outs,r,rows", [(1406, [1024, 256, 256], 64, False), (12792, [4096, 4096, 4096], 128, False), (1353, [1408], 256, True),
                                           (12792, [11008, 11008], 128, False), (700, [128], 128, False), (517, [768, 640], 64, True)])
def test_lora_rows_v(hip, M, outs, r, rows):
    """vlr_lora_rows_v: v_t = dy[:, ofs_t .. + out_t] B_t (grouped-query widths differ per target), fp32 torch reference."""
    n, tot = len(outs), sum(outs)
    dy = rnd(M, tot, seed=3)
    B = rnd(tot, r, seed=4, scale=0.05)
    rowmask = None
    if rows:
        g = torch.Generator().manual_seed(6)
        rm = (torch.rand(M, generator=g) < 0.5)
        rm[0:128] = False
        rowmask = rm.to(torch.uint8).to(DEV)
    v = torch.full((M, n * r), float("nan"), dtype=torch.bfloat16, device=DEV)
    o = torch.tensor(outs, dtype=torch.int32)          # host array
    hip.call("vlr_lora_rows_v", n, dy, tot, o, B, v, n * r, M, r, rowmask)
    torch.cuda.synchronize()
    ofs = 0
    for t in range(n):
        ref = dy[:, ofs:ofs + outs[t]].float() @ B[ofs:ofs + outs[t]].float()
        if rows:
            ref = ref * rowmask.float().view(-1, 1)
        check(v[:, t * r:(t + 1) * r], ref, 8e-3, f"v of target {t}")
        ofs += outs[t]
    assert torch.isfinite(v.float()).all()


@pytest.mark.gpu
@pytest.mark.parametrize("M,in_,r,n,p", [(1000, 512, 64, 2, 0.25), (1353, 1024, 256, 1, 0.05)])
def test_adapter_products_restricted_to_a_row_set(hip, M, in_, r, n, p):
    """PLoRA acts on the image rows only: the row-set forms (vlr_gemm_grouped_bits_rows, vlr_gemm_dropout_acc_multi_rows) skip the 128-row
    tiles / 64-row slabs without a marked row and are BIT-IDENTICAL to the dense calls followed by vlr_rows_mask.  The row set has marked
    runs that start and end inside tiles, whole unmarked tiles (skipped) and a ragged last tile."""
    from vlrlhf import _hip as HH
    HH.ensure_splitk_workspace(DEV, force=True)
    seed, alpha, scale = 7, 2.0 / (1 - p), 2.0
    rowmask = torch.zeros(M, dtype=torch.uint8, device=DEV)
    rowmask[70:200] = 1
    rowmask[640:705] = 1
    rowmask[M - 3:] = 1
    gstride = M * in_ // 8
    bits = torch.zeros(n * gstride, dtype=torch.uint8, device=DEV)
    for t in range(n):
        hip.call("vlr_dropout_bits", bits[t * gstride:], M * in_, p, seed + t)
    x = rnd(M, in_, seed=1)
    A = rnd(n * r, in_, seed=2, scale=0.05)
    ldu = n * r
    poison = lambda: torch.full((M, ldu), float("nan"), dtype=torch.bfloat16, device=DEV)      # noqa: E731  (a skipped tile keeps what was there)
    u0, u1 = poison(), poison()
    hip.call("vlr_gemm_grouped_bits", 0, x, A, u0, M, r, in_, in_, in_, ldu, n, 0, r * in_, r, alpha, 0, 1, seed, p, in_, bits, gstride)
    hip.call("vlr_gemm_grouped_bits_rows", 0, x, A, u1, M, r, in_, in_, in_, ldu, n, 0, r * in_, r, alpha, 0, 1, seed, p, in_, bits, gstride, rowmask)
    torch.cuda.synchronize()
    if in_ < 1024:          # (K >= 1024 splits along K: the reduction then writes the skipped tile's rows from untouched partials)
        assert bool(torch.isnan(u1[256:384].float()).all()), "rows 256..383 hold no marked row: the tile must not have been computed"
    for u in (u0, u1):
        hip.call("vlr_rows_mask", u, ldu, ldu, rowmask, M)
    torch.cuda.synchronize()
    assert torch.equal(u0, u1) and float(u1.float().abs().sum()) > 0, "u = drop(x) A^T on the row set"
    # v = dy B (layout 1) on the row set
    out = 384
    dy, B = rnd(M, out, seed=5), rnd(out, r, seed=6, scale=0.05)
    v0 = torch.full((M, r), float("nan"), dtype=torch.bfloat16, device=DEV)
    v1 = v0.clone()
    hip.call("vlr_gemm_grouped", 1, dy, B, v0, M, r, out, out, r, r, 1, 0, 0, 0, 1.0, 0, 0, 0, 0.0, 0)
    hip.call("vlr_gemm_grouped_bits_rows", 1, dy, B, v1, M, r, out, out, r, r, 1, 0, 0, 0, 1.0, 0, 0, 0, 0.0, 0, None, 0, rowmask)
    for v_ in (v0, v1):
        hip.call("vlr_rows_mask", v_, r, r, rowmask, M)
    torch.cuda.synchronize()
    assert torch.equal(v0, v1) and float(v1.float().abs().sum()) > 0, "v = dy B on the row set"
    # dx += mask . (v A) with zero v rows outside the row set
    v = rnd(M, n * r, seed=3, scale=0.5)
    hip.call("vlr_rows_mask", v, n * r, n * r, rowmask, M)
    dx0 = rnd(M, in_, seed=4)
    a0, a1 = dx0.clone(), dx0.clone()
    hip.call("vlr_gemm_dropout_acc_multi_bits", n, v, n * r, A, a0, M, in_, r, p, seed, scale, 1, bits, gstride)
    hip.call("vlr_gemm_dropout_acc_multi_rows", n, v, n * r, A, a1, M, in_, r, p, seed, scale, 1, bits, gstride, rowmask)
    torch.cuda.synchronize()
    assert torch.equal(a0, a1), "dx += mask . (v A) on the row set"
    assert torch.equal(a1[rowmask == 0], dx0[rowmask == 0]) and not torch.equal(a1, dx0)


@pytest.mark.gpu
@pytest.mark.parametrize("M,in_,r,out,p", [(1024, 512, 64, 384, 0.25), (4096, 1024, 256, 512, 0.05)])
def test_adapter_gradient_reductions_over_a_k_tile_list(hip, M, in_, r, out, p):
    """PLoRA's dB = dy^T u and dA = v^T drop(x) contract over the token rows; u and v are zero outside the image rows, so
    vlr_gemm_grouped_bits_ktiles reads only the 64-row K tiles of vlr_rows_tile_list.  Same product as the dense call (fp32 accumulation,
    another split-K partition: compared at rounding level) - and NaN-poisoned operand rows in the unlisted tiles prove they are not read."""
    from vlrlhf import _hip as HH
    HH.ensure_splitk_workspace(DEV, force=True)
    rowmask = torch.zeros(M, dtype=torch.uint8, device=DEV)
    rowmask[70:200] = 1
    rowmask[640:705] = 1
    rowmask[M - 3:] = 1
    tl = torch.full((M // 64 + 2,), -1, dtype=torch.int32, device=DEV)
    hip.call("vlr_rows_tile_list", rowmask, M, tl)
    torch.cuda.synchronize()
    want = rowmask.view(-1, 64).any(1).nonzero().flatten().to(torch.int32)
    assert int(tl[0]) == want.numel() and torch.equal(tl[1:1 + want.numel()], want), tl[:8]
    listed = torch.zeros(M, dtype=torch.bool, device=DEV)
    listed.view(-1, 64)[want.long()] = True
    seed, alpha = 11, 2.0 / (1 - p)
    dy, u = rnd(M, out, seed=1), rnd(M, r, seed=2, scale=0.5)
    hip.call("vlr_rows_mask", u, r, r, rowmask, M)
    dB0 = torch.zeros(out, r, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_grouped", 2, dy, u, dB0, out, r, M, out, r, r, 1, 0, 0, 0, 1.0, 0, 0, 0, 0.0, 0)
    dyp, up = dy.clone(), u.clone()
    dyp[~listed] = float("nan")
    up[~listed] = float("nan")
    dB1 = torch.zeros(out, r, dtype=torch.bfloat16, device=DEV)
    hip.call("vlr_gemm_grouped_bits_ktiles", 2, dyp, up, dB1, out, r, M, out, r, r, 1, 0, 0, 0, 1.0, 0, 0, 0, 0.0, 0, None, 0, tl)
    torch.cuda.synchronize()
    ref = dy.float().t() @ u.float()
    check(dB1, ref, 8e-3, "dB over the K-tile list")
    assert float((dB0.float() - dB1.float()).abs().max()) <= 0.01 * float(ref.abs().max())
    # dA with the K-tile-blocked transposed masks
    gstride, tstride = M * in_ // 8, HH.helper("vlr_dropout_bits_kt_bytes", M, in_)
    bits_rm = torch.zeros(gstride, dtype=torch.uint8, device=DEV)
    bits_kt = torch.zeros(tstride, dtype=torch.uint8, device=DEV)
    hip.call("vlr_dropout_bits2", bits_rm, bits_kt, M, in_, p, seed)
    x, v = rnd(M, in_, seed=3), rnd(M, r, seed=4, scale=0.5)
    hip.call("vlr_rows_mask", v, r, r, rowmask, M)
    xp, vp = x.clone(), v.clone()
    xp[~listed] = float("nan")
    vp[~listed] = float("nan")
    dA0, dA1 = (torch.zeros(r, in_, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    hip.call("vlr_gemm_grouped_bits", 2, v, x, dA0, r, in_, M, r, in_, in_, 1, 0, 0, 0, alpha, 0, 3, seed, p, in_, bits_kt, tstride)
    hip.call("vlr_gemm_grouped_bits_ktiles", 2, vp, xp, dA1, r, in_, M, r, in_, in_, 1, 0, 0, 0, alpha, 0, 3, seed, p, in_, bits_kt, tstride, tl)
    torch.cuda.synchronize()
    mk = ((bits_rm.view(-1, 1) >> torch.arange(8, device=DEV, dtype=torch.uint8)) & 1).reshape(M, in_).float()
    ref = alpha * v.float().t() @ (x.float() * mk)
    check(dA1, ref, 8e-3, "dA over the K-tile list")
    assert float((dA0.float() - dA1.float()).abs().max()) <= 0.01 * float(ref.abs().max())
    # an empty list writes zeros
    hip.call("vlr_rows_tile_list", torch.zeros(M, dtype=torch.uint8, device=DEV), M, tl)
    dB1.fill_(1.0)
    hip.call("vlr_gemm_grouped_bits_ktiles", 2, dyp, up, dB1, out, r, M, out, r, r, 1, 0, 0, 0, 1.0, 0, 0, 0, 0.0, 0, None, 0, tl)
    torch.cuda.synchronize()
    assert int(tl[0]) == 0 and float(dB1.float().abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------- 128x128 ring kernel, other ring depths
_RING_PROBE = r"""
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
from vlrlhf import _hip
_hip.ensure_splitk_workspace("cuda", force=True)
g = torch.Generator().manual_seed(0)
rn = lambda *s: (torch.randn(*s, generator=g) * 0.5).bfloat16().cuda()
worst = 0.0
for layout, (M, N, K) in [(0, (504, 1024, 4096)), (1, (504, 1024, 4096)), (2, (1024, 512, 5000)), (0, (200, 136, 72)), (1, (300, 264, 1000)), (2, (136, 200, 777 * 4))]:
    a = rn(M, K) if layout != 2 else rn(K, M)
    b = rn(N, K) if layout == 0 else rn(K, N)
    c = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    lda = K if layout != 2 else M
    ldb = K if layout == 0 else N
    _hip.call("vlr_gemm_bf16", layout, a, b, c, None, None, M, N, K, lda, ldb, N, 0, 0, 0, 0)
    A = a.float() if layout != 2 else a.float().t()
    B = b.float().t() if layout == 0 else b.float()
    ref = A @ B
    torch.cuda.synchronize()
    worst = max(worst, float((c.float() - ref).abs().max()) / float(ref.abs().max()))
print("WORST", worst)
"""


@pytest.mark.parametrize("depth", ["3", "4", "0"])
def test_gemm128_ring_depths(depth):
    """VLR_GEMM128P is read once per process: the ring depths the default (2) does not use, and the register-staged kernel (0), in a child
    process each - NT / NN / TN, split along K and not, ragged edges and a K tail."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VLR_GEMM128P=depth)
    r = subprocess.run([sys.executable, "-c", _RING_PROBE, root, os.path.join(root, "vl-rlhf_amd")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    worst = float(r.stdout.strip().splitlines()[-1].split()[1])
    assert worst < 8e-3, (depth, worst)


# ---------------------------------------------------------------------------------------------------- 64-query forward attention kernel
def test_fwd3_kernel_in_child_process():
    """VLR_ATTN_FWD3 is read once per process: every attention test of this file (forward parity incl. masks / GQA / the step's sizes,
    and the backward tests, which consume the forward's lse) again in a child process on attn_fwd3_kernel (csrc/attn_fwd3.h: 64 queries
    per wave, asm-owned accumulator registers, explicit issue order; opt-in - it is not faster than the 32-query kernel yet)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VLR_ATTN_FWD3="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_hip_kernels.py"), "-k", "attention", "-x", "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-1000:]
