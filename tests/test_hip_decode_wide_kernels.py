"""The wide skinny GEMM (csrc/decode.hip: vlr_gemv_wide_bf16, vlr_gemv_wide_bf16_lora - up to 64 rows in one pass over the weights)
through the C ABI on the MI355X.  The yardstick is the 16-row entry point itself, called on rows [0, 16), [16, 32), ... of the same X
(pos, residual and Y advanced by the same rows): the wide call must give the SAME BITS, so no tolerance appears anywhere in this file.
That the 16-row calls are right is the business of tests/test_hip_decode_kernels.py and tests/test_hip_decode_lora_kernels.py.
Outputs are NaN-filled before every call and are taller than M: the rows beyond M must stay NaN.
The decoder layer is run at batch 33 twice - scratch sized by the wide helpers (64-row groups) and scratch sized for 16 rows (the
16-row groups of every existing caller) - and must write the same bits.  Needs a real MI355X:  pytest -m gpu"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, F32RES, ROPE, SWIGLU = 0, 1, 2, 3, 4               # VLR_GEMV_* modes (include/vlr.h)
MAX_POS = 512
MMAX, TALL = 64, 3                                            # inputs are built for 64 rows; Y has TALL more rows than M
# a ragged last k chunk and a ragged column block; several K slices over one column block; two true 7B shapes (q|k|v, down)
SHAPES = [(136, 72), (1024, 64), (4096, 12288), (11008, 4096)]
ROWS = [5, 17, 31, 32, 33, 48, 64]                            # M = 5: one row tile must still work


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return _hip


def rnd(*shape, scale=1.0, seed=0, dtype=torch.bfloat16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(dtype)


def rope_dims(N):
    """(head_dim, rope_cols): rotated heads over about two thirds of the columns, the rest plain (the v block)"""
    hd = 128 if N % 128 == 0 else 16
    return hd, (2 * N // 3) // hd * hd


_INPUTS = {}


def inputs(K, N):
    """device inputs of one shape for 64 rows, built once and never written"""
    if (K, N) not in _INPUTS:
        hd, _ = rope_dims(N)
        inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd))
        ang = torch.arange(MAX_POS, dtype=torch.float64)[:, None] * inv[None, :]
        _INPUTS[(K, N)] = dict(
            X=rnd(MMAX, K, seed=K + N), W=rnd(N, K, scale=1 / math.sqrt(K), seed=K + N + 1), bias=rnd(N, seed=K + N + 2),
            res=rnd(MMAX, N, seed=K + N + 3), res32=rnd(MMAX, N, seed=K + N + 4, dtype=torch.float32),
            # a different position in every row: 37 is odd, so rows 16 .. 63 repeat none of rows 0 .. 15
            pos=torch.tensor([(37 * m + 5) % MAX_POS for m in range(MMAX)], dtype=torch.int32, device=DEV),
            cos=ang.cos().float().to(DEV), sin=ang.sin().float().to(DEV))
    return _INPUTS[(K, N)]


def fresh_output(mode, c, M, N):
    """NaN everywhere, TALL rows more than M; F32RES runs in place on the fp32 residual stream: its first M rows hold it"""
    if mode in (F32, F32RES):
        Y = torch.full((M + TALL, N), float("nan"), dtype=torch.float32, device=DEV)
        if mode == F32RES:
            Y[:M] = c["res32"][:M]
        return Y
    return torch.full((M + TALL, N // 2 if mode == SWIGLU else N), float("nan"), dtype=torch.bfloat16, device=DEV)


def gemv(hip, fn, mode, c, Y, m0, mr, N, K, ws, adapter=None):
    """one call of entry point `fn` on rows m0 .. m0 + mr - 1"""
    hd, rc = rope_dims(N)
    bias = c["bias"] if mode in (BF16, ROPE) else None
    res, ldr = (c["res"][m0:], N) if mode == BF16 else ((Y[m0:], N) if mode == F32RES else (None, 0))
    pos = c["pos"][m0:] if mode == ROPE else None
    args = (mode, c["X"][m0:], K, c["W"], Y[m0:], Y.shape[1], bias, res, ldr, pos, c["cos"] if mode == ROPE else None,
            c["sin"] if mode == ROPE else None, rc if mode == ROPE else 0, hd, MAX_POS, mr, N, K, ws)
    hip.call(fn, *args, *(adapter or ()))


def scratch(nbytes):
    assert nbytes > 0
    return torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=DEV)


def same_bits(a, b, what):
    assert torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                       b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)), what


def check_rows(Y, ref, M, what):
    assert torch.isfinite(Y[:M].float()).all(), f"{what}: a row below M was not written"
    assert torch.isnan(Y[M:].float()).all(), f"{what}: a row beyond M was written"
    same_bits(Y, ref, what)


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("mode", [ROPE, SWIGLU, BF16, F32RES, F32])
def test_wide_equals_16_row_groups(hip, mode, K, N, M):
    """q|k|v + bias + RoPE at a different position per row, SwiGLU, bf16 + bias + residual, the fp32 stream in place, fp32 logits"""
    c = inputs(K, N)
    lib = hip.lib()
    ref = fresh_output(mode, c, M, N)
    ws16 = scratch(int(lib.vlr_gemv_workspace_bytes(min(M, 16), N, K)))
    for m0 in range(0, M, 16):
        gemv(hip, "vlr_gemv_bf16", mode, c, ref, m0, min(16, M - m0), N, K, ws16)
    Y = fresh_output(mode, c, M, N)
    gemv(hip, "vlr_gemv_wide_bf16", mode, c, Y, 0, M, N, K, scratch(int(lib.vlr_gemv_wide_workspace_bytes(M, N, K))))
    torch.cuda.synchronize()
    check_rows(Y, ref, M, f"mode {mode} K {K} N {N} M {M}")


def lora_outs(T, N):
    """unequal row blocks whose edges fall inside a 64-column block"""
    return {1: (N,), 2: (N // 2 + 20, N - N // 2 - 20), 3: (N // 2 + 4, N // 4 + 6, N - N // 2 - N // 4 - 10)}[T]


_ADAPTERS = {}


def adapter_of(K, N, T, r):
    if (K, N, T, r) not in _ADAPTERS:
        _ADAPTERS[(K, N, T, r)] = (rnd(T * r, K, scale=1 / math.sqrt(K), seed=7 * r + T), rnd(N, r, scale=0.5, seed=7 * r + T + 1))
    return _ADAPTERS[(K, N, T, r)]


# (mode, targets, pass the row split): q|k|v in three unequal blocks under RoPE, two unequal blocks, gate|up (equal halves, the
# split left to the library), one target on the fp32 stream
LORA_FORMS = [(ROPE, 3, True), (BF16, 2, True), (SWIGLU, 2, False), (F32RES, 1, False)]


@pytest.mark.parametrize("M", [17, 33, 64])
@pytest.mark.parametrize("K,N", [(136, 200), (4096, 12288)])
@pytest.mark.parametrize("r", [8, 64, 264])
@pytest.mark.parametrize("mode,T,split", LORA_FORMS)
def test_wide_lora_equals_16_row_groups(hip, mode, T, split, r, K, N, M):
    """the live adapter: x A^T through the wide kernel, the adapter slice over the row tiles; r = 264 walks the rank in two LDS chunks
    where a block spans two targets"""
    c = inputs(K, N)
    A, B = adapter_of(K, N, T, r)
    outs = (hip.C.c_int * T)(*lora_outs(T, N)) if split else None
    lib = hip.lib()
    ref = fresh_output(mode, c, M, N)
    ws16 = scratch(int(lib.vlr_gemv_lora_workspace_bytes(16, N, K, T * r)))
    u16 = scratch(int(lib.vlr_gemv_lora_u_bytes(16, K, T * r)))
    for m0 in range(0, M, 16):
        gemv(hip, "vlr_gemv_bf16_lora", mode, c, ref, m0, min(16, M - m0), N, K, ws16, (A, B, r, T, outs, 0.25, u16))
    Y = fresh_output(mode, c, M, N)
    ws = scratch(int(lib.vlr_gemv_wide_lora_workspace_bytes(M, N, K, T * r)))
    u = scratch(int(lib.vlr_gemv_wide_lora_u_bytes(M, K, T * r)))
    gemv(hip, "vlr_gemv_wide_bf16_lora", mode, c, Y, 0, M, N, K, ws, (A, B, r, T, outs, 0.25, u))
    torch.cuda.synchronize()
    check_rows(Y, ref, M, f"mode {mode} targets {T} r {r} K {K} N {N} M {M}")
    plain = fresh_output(mode, c, M, N)
    gemv(hip, "vlr_gemv_wide_bf16", mode, c, plain, 0, M, N, K, ws)
    torch.cuda.synchronize()
    assert not torch.equal(Y[:M], plain[:M]), "the adapter changes the result"


@pytest.mark.parametrize("K,N", [(136, 200), (4096, 12288)])
@pytest.mark.parametrize("mode,T,split", LORA_FORMS)
def test_wide_lora_zero_b_and_null_adapter_are_the_plain_call(hip, mode, T, split, K, N):
    """B = 0 adds 0.0f last, A = B = NULL makes the adapter-free wide call: both its bits"""
    M, r = 33, 64
    c = inputs(K, N)
    A, B = adapter_of(K, N, T, r)
    outs = (hip.C.c_int * T)(*lora_outs(T, N)) if split else None
    lib = hip.lib()
    ws = scratch(int(lib.vlr_gemv_wide_lora_workspace_bytes(M, N, K, T * r)))
    u = scratch(int(lib.vlr_gemv_wide_lora_u_bytes(M, K, T * r)))
    plain, zero, null = (fresh_output(mode, c, M, N) for _ in range(3))
    gemv(hip, "vlr_gemv_wide_bf16", mode, c, plain, 0, M, N, K, ws)
    gemv(hip, "vlr_gemv_wide_bf16_lora", mode, c, zero, 0, M, N, K, ws, (A, torch.zeros_like(B), r, T, outs, 0.25, u))
    gemv(hip, "vlr_gemv_wide_bf16_lora", mode, c, null, 0, M, N, K, ws, (None, None, r, T, outs, 0.25, u))
    torch.cuda.synchronize()
    check_rows(zero, plain, M, "B = 0")
    check_rows(null, plain, M, "NULL adapter")


def test_argument_errors_launch_nothing(hip):
    """M = 0 and M = 65 are VLR_ERR_ARG with the row rule in the text, the NaN-filled output is untouched; the 16-row entry points keep
    their own rule"""
    K, N, r = 136, 72, 8
    c = inputs(K, N)
    A, B = adapter_of(K, N, 1, r)
    lib = hip.lib()
    ws = scratch(int(lib.vlr_gemv_wide_lora_workspace_bytes(64, N, K, r)))
    u = scratch(int(lib.vlr_gemv_wide_lora_u_bytes(64, K, r)))
    Y = torch.full((MMAX + TALL, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    X = torch.cat([c["X"], c["X"][:TALL]])                   # 67 readable rows
    for M in (0, 65):
        with pytest.raises(ValueError, match="1 <= M <= 64"):
            hip.call("vlr_gemv_wide_bf16", BF16, X, K, c["W"], Y, N, None, None, 0, None, None, None, 0, 16, MAX_POS, M, N, K, ws)
        with pytest.raises(ValueError, match="1 <= M <= 64"):
            hip.call("vlr_gemv_wide_bf16_lora", BF16, X, K, c["W"], Y, N, None, None, 0, None, None, None, 0, 16, MAX_POS, M, N, K, ws,
                     A, B, r, 1, None, 1.0, u)
    with pytest.raises(ValueError, match="1 <= M <= 16"):
        hip.call("vlr_gemv_bf16", BF16, X, K, c["W"], Y, N, None, None, 0, None, None, None, 0, 16, MAX_POS, 17, N, K, ws)
    with pytest.raises(ValueError, match="1 <= M <= 16"):
        hip.call("vlr_gemv_bf16_lora", BF16, X, K, c["W"], Y, N, None, None, 0, None, None, None, 0, 16, MAX_POS, 17, N, K, ws, A, B, r, 1,
                 None, 1.0, u)
    torch.cuda.synchronize()
    assert torch.isnan(Y.float()).all()


def test_workspace_helpers(hip):
    lib = hip.lib()
    for K, N in SHAPES:
        for M in (1, 16):
            assert lib.vlr_gemv_wide_workspace_bytes(M, N, K) == lib.vlr_gemv_workspace_bytes(M, N, K) > 0
        assert lib.vlr_gemv_wide_workspace_bytes(64, N, K) == 4 * lib.vlr_gemv_workspace_bytes(16, N, K)
        assert lib.vlr_gemv_wide_workspace_bytes(200, N, K) == lib.vlr_gemv_wide_workspace_bytes(64, N, K)


# ---- the decoder layer at batch 33: 64-row groups (wide scratch) against the 16-row groups (scratch sized for 16 rows)
_LAYERS = {}


def layer_case(hip, H, I, nh, nkv):
    if (H, I, nh, nkv) in _LAYERS:
        return _LAYERS[(H, I, nh, nkv)]
    hd, max_pos, B, S, r = 128, 512, 33, 20, 16
    Nq, Nkv = nh * hd, nkv * hd
    N = Nq + 2 * Nkv
    cos = torch.empty(max_pos, hd // 2, dtype=torch.float32, device=DEV)
    sin = torch.empty_like(cos)
    hip.call("vlr_rope_table", cos, sin, max_pos, hd, 10000.0)
    sc = 1.0 / math.sqrt(H)
    W = dict(ln1=(1 + 0.1 * rnd(H, seed=20).float()).bfloat16(), wqkv=rnd(N, H, scale=sc, seed=21), wo=rnd(H, Nq, scale=sc, seed=22),
             ln2=(1 + 0.1 * rnd(H, seed=23).float()).bfloat16(), wgu=rnd(2 * I, H, scale=sc, seed=24),
             wdown=rnd(H, I, scale=1 / math.sqrt(I), seed=25), bqkv=rnd(N, scale=0.1, seed=26))
    Ad = dict(a_qkv=rnd(3 * r, H, scale=sc, seed=30), b_qkv=rnd(N, r, scale=0.3, seed=31), a_o=rnd(r, Nq, scale=sc, seed=32),
              b_o=rnd(H, r, scale=0.3, seed=33), a_gu=rnd(2 * r, H, scale=sc, seed=34), b_gu=rnd(2 * I, r, scale=0.3, seed=35),
              a_down=rnd(r, I, scale=1 / math.sqrt(I), seed=36), b_down=rnd(H, r, scale=0.3, seed=37))
    cap = S + 4
    km = torch.zeros(B, cap, dtype=torch.int32, device=DEV)
    km[:, :S + 1] = 1
    for b in range(B):
        km[b, :b % 7] = 0                                     # left padding of unequal lengths
    c = dict(H=H, I=I, nh=nh, nkv=nkv, hd=hd, B=B, S=S, r=r, cap=cap, Nq=Nq, N=N, W=W, Ad=Ad, cos=cos, sin=sin, km=km, max_pos=max_pos,
             pos=(km[:, :S].sum(1)).to(torch.int32).contiguous(),      # every row at its own position
             kc=rnd(B, nkv, cap, hd, seed=40), vc=rnd(B, nkv, cap, hd, seed=41), x=rnd(B, H, seed=42, dtype=torch.float32))
    _LAYERS[(H, I, nh, nkv)] = c
    return c


def run_layer(hip, c, resid_f32, lora, wide):
    """one decode step of the layer at column S -> (x_inout, the K column, the V column written)"""
    H, I, nh, nkv, B, N, Nq, r = (c[k] for k in ("H", "I", "nh", "nkv", "B", "N", "Nq", "r"))
    lib = hip.lib()
    cfg = hip.LlamaCfg(H, I, nh, c["hd"], 1e-5, c["max_pos"], c["cos"].data_ptr(), c["sin"].data_ptr(), nkv, resid_f32)
    lw = hip.LayerWeights(*(c["W"][k].data_ptr() for k in ("ln1", "wqkv", "wo", "ln2", "wgu", "wdown", "bqkv")))
    shapes, rt = ((N, H), (H, Nq), (2 * I, H), (H, I)), (3 * r, r, 2 * r, r)
    mb = min(B, 64) if wide else 16
    if lora:
        fw, fu = (lib.vlr_gemv_wide_lora_workspace_bytes, lib.vlr_gemv_wide_lora_u_bytes) if wide else \
            (lib.vlr_gemv_lora_workspace_bytes, lib.vlr_gemv_lora_u_bytes)
        gb = max(int(fw(mb, n, k, t)) for (n, k), t in zip(shapes, rt))
        ub = max(int(fu(mb, k, t)) for (n, k), t in zip(shapes, rt))
    else:
        fw = lib.vlr_gemv_wide_workspace_bytes if wide else lib.vlr_gemv_workspace_bytes
        gb, ub = max(int(fw(mb, n, k)) for n, k in shapes), 0
    ab = int(lib.vlr_attn_decode_workspace_bytes(B, nh, c["cap"]))
    d = dict(xn=torch.empty(B, H, dtype=torch.bfloat16, device=DEV), rstd=torch.empty(B, device=DEV),
             qkv=torch.empty(B, N, dtype=torch.bfloat16, device=DEV), attn=torch.empty(B, Nq, dtype=torch.bfloat16, device=DEV),
             act=torch.empty(B, I, dtype=torch.bfloat16, device=DEV), gemv=scratch(gb), attn_ws=torch.empty(ab, dtype=torch.uint8, device=DEV))
    dws = hip.DecodeWs(d["xn"].data_ptr(), d["rstd"].data_ptr(), d["qkv"].data_ptr(), d["attn"].data_ptr(), d["act"].data_ptr(),
                       d["gemv"].data_ptr(), gb, d["attn_ws"].data_ptr(), ab)
    x = c["x"].to(torch.float32 if resid_f32 else torch.bfloat16).clone()
    kc, vc = c["kc"].clone(), c["vc"].clone()
    kc[:, :, c["S"]:] = float("nan")
    vc[:, :, c["S"]:] = float("nan")
    if lora:
        u = scratch(ub)
        lws = hip.DecodeLoraWs(u.data_ptr(), ub)
        lo = hip.LoraWeights(r, 2.0, 0.0, *(c["Ad"][k].data_ptr() for k in ("a_qkv", "b_qkv", "a_o", "b_o", "a_gu", "b_gu", "a_down", "b_down")),
                             3, None)
        hip.call("vlr_decoder_layer_decode_lora", cfg, lw, lo, dws, lws, x, c["pos"], kc, vc, c["km"], B, c["cap"], c["S"])
    else:
        hip.call("vlr_decoder_layer_decode", cfg, lw, dws, x, c["pos"], kc, vc, c["km"], B, c["cap"], c["S"])
    torch.cuda.synchronize()
    assert torch.isnan(kc[:, :, c["S"] + 1:].float()).all()
    return x, kc[:, :, c["S"]].clone(), vc[:, :, c["S"]].clone()


@pytest.mark.parametrize("lora", [False, True])
@pytest.mark.parametrize("resid_f32", [0, 1])
@pytest.mark.parametrize("H,I,nh,nkv", [(256, 256, 2, 1), (4096, 11008, 32, 32)])
def test_decoder_layer_decode_wide_scratch_equals_16_row_groups(hip, H, I, nh, nkv, resid_f32, lora):
    c = layer_case(hip, H, I, nh, nkv)
    xw, kw, vw = run_layer(hip, c, resid_f32, lora, wide=True)
    xg, kg, vg = run_layer(hip, c, resid_f32, lora, wide=False)
    assert torch.isfinite(xw.float()).all() and torch.isfinite(kw.float()).all() and torch.isfinite(vw.float()).all()
    assert not torch.equal(xw.float(), c["x"]), "the layer moved the stream"
    same_bits(xw, xg, "x_inout")
    same_bits(kw, kg, "the new K column")
    same_bits(vw, vg, "the new V column")
