"""The wide skinny GEMM over packed int4 weights (csrc/decode.hip: vlr_gemv_wide_w4, vlr_gemv_wide_w4_lora - up to 64 rows in one pass
over the packed words) through the C ABI on the MI355X.  The yardstick is the 16-row entry point itself (vlr_gemv_w4, vlr_gemv_w4_lora),
called on rows [0, 16), [16, 32), ... of the same X (pos, residual and Y advanced by the same rows): the wide call must give the SAME
BITS, so no tolerance appears in those tests.  That the 16-row calls are right is the business of tests/test_hip_gptq.py and
tests/test_hip_decode_lora_kernels.py; one case here is held against the fp64 product on the dequantised matrix all the same, under the
bound tests/test_hip_gptq.py::test_gemv_w4_plain sets for fp32 output.  Outputs are NaN-filled before every call and are taller than
M: the rows beyond M must stay NaN.  The packed decoder layer is run at batch 33 twice - scratch sized by the wide helpers and scratch
sized for 16 rows - and must write the same bits.  Needs a real MI355X:  pytest -m gpu"""
import inspect
import math
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gptq_ref as R  # noqa: E402
from tests import test_hip_gptq as G  # noqa: E402
from tests.test_hip_decode_wide_kernels import (BF16, DEV, F32, F32RES, MAX_POS, MMAX, ROPE, SWIGLU, check_rows, fresh_output,  # noqa: E402
                                                 lora_outs, rnd, rope_dims, same_bits, scratch)

# (N, K, group): one chunk and one workgroup; a column edge inside the second 64-column half, a K tail of 32 and scales read per 32-k
# step; two column blocks with one group per chunk; several K slices
SHAPES = [(128, 128, 128), (136, 416, 32), (192, 512, 128), (256, 8192, 128)]
ROWS = [1, 16, 17, 31, 32, 33, 48, 49, 64]


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return _hip


_INPUTS = {}


def inputs(N, K, g):
    """device inputs of one shape for 64 rows, built once and never written: the packed linear of tests/test_hip_gptq.py (zeros 1 .. 16,
    an all-15 and an all-0 column) and its dequantised W"""
    if (N, K, g) not in _INPUTS:
        hd, _ = rope_dims(N)
        inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd))
        ang = torch.arange(MAX_POS, dtype=torch.float64)[:, None] * inv[None, :]
        _INPUTS[(N, K, g)] = dict(
            G.packed_case(K, N, g), g=R.group(K, g), X=rnd(MMAX, K, seed=K + N), bias=rnd(N, seed=K + N + 2), res=rnd(MMAX, N, seed=K + N + 3),
            res32=rnd(MMAX, N, seed=K + N + 4, dtype=torch.float32),
            pos=torch.tensor([(37 * m + 5) % MAX_POS for m in range(MMAX)], dtype=torch.int32, device=DEV),
            cos=ang.cos().float().to(DEV), sin=ang.sin().float().to(DEV))
    return _INPUTS[(N, K, g)]


def gemv(hip, fn, mode, c, Y, m0, mr, N, K, ws, adapter=None, rope=None):
    """one call of the packed entry point `fn` on rows m0 .. m0 + mr - 1; rope: (head_dim, rope_cols) instead of rope_dims(N)"""
    hd, rc = rope or rope_dims(N)
    bias = c["bias"] if mode in (BF16, ROPE) else None
    res, ldr = (c["res"][m0:], N) if mode == BF16 else ((Y[m0:], N) if mode == F32RES else (None, 0))
    pos = c["pos"][m0:] if mode == ROPE else None
    args = (mode, c["X"][m0:], K, c["qweight"], c["qzeros"], c["scales"], c["g"], Y[m0:], Y.shape[1], bias, res, ldr, pos,
            c["cos"] if mode == ROPE else None, c["sin"] if mode == ROPE else None, rc if mode == ROPE else 0, hd, MAX_POS, mr, N, K, ws)
    hip.call(fn, *args, *(adapter or ()))


@pytest.mark.parametrize("N,K,g", SHAPES)
@pytest.mark.parametrize("mode", [ROPE, SWIGLU, BF16, F32RES, F32])
def test_wide_w4_equals_16_row_groups(hip, mode, N, K, g):
    """q|k|v + bias + RoPE at a different position per row, SwiGLU, bf16 + bias + residual, the fp32 stream in place, fp32 out - at every
    row count at which the number of row tiles or the last tile's fill changes"""
    c = inputs(N, K, g)
    lib = hip.lib()
    for M in ROWS:
        ref = fresh_output(mode, c, M, N)
        ws16 = scratch(int(lib.vlr_gemv_w4_workspace_bytes(min(M, 16), N, K)))
        for m0 in range(0, M, 16):
            gemv(hip, "vlr_gemv_w4", mode, c, ref, m0, min(16, M - m0), N, K, ws16)
        Y = fresh_output(mode, c, M, N)
        gemv(hip, "vlr_gemv_wide_w4", mode, c, Y, 0, M, N, K, scratch(int(lib.vlr_gemv_wide_w4_workspace_bytes(M, N, K))))
        torch.cuda.synchronize()
        check_rows(Y, ref, M, f"mode {mode} N {N} K {K} group {g} M {M}")


def test_wide_w4_against_the_fp64_dequantised_product(hip):
    """33 rows, several K slices, fp32 out: the fp64 product of X and the dequantised matrix of tests/gptq_ref.py under the bound
    test_gemv_w4_plain holds the 16-row kernel's fp32 output to (read from that test, not restated)"""
    m = re.search(r'check\(F, ref, ([0-9.e+-]+), "fp32 out"\)', inspect.getsource(G.test_gemv_w4_plain))
    assert m, "tests/test_hip_gptq.py::test_gemv_w4_plain no longer states its fp32 bound where this test reads it"
    bound = float(m.group(1))
    N, K, g, M = 256, 8192, 128, 33
    c = inputs(N, K, g)
    W = R.dequant(c["qweight"], c["qzeros"], c["scales"], g)
    assert torch.equal(W, c["W"])
    ref = (c["X"][:M].double() @ W.double().T)
    Y = fresh_output(F32, c, M, N)
    gemv(hip, "vlr_gemv_wide_w4", F32, c, Y, 0, M, N, K, scratch(int(hip.lib().vlr_gemv_wide_w4_workspace_bytes(M, N, K))))
    torch.cuda.synchronize()
    G.check(Y[:M].double(), ref, bound, f"wide int4, fp32 out, M {M} N {N} K {K} against fp64")


_ADAPTERS = {}


def adapter_of(K, N, T, r):
    if (K, N, T, r) not in _ADAPTERS:
        _ADAPTERS[(K, N, T, r)] = (rnd(T * r, K, scale=1 / math.sqrt(K), seed=7 * r + T), rnd(N, r, scale=0.5, seed=7 * r + T + 1))
    return _ADAPTERS[(K, N, T, r)]


def lora_pair(hip, mode, c, M, N, K, T, r, outs, rope=None, B=None):
    """(wide call, the same rows in 16-row groups) with the live adapter"""
    A, B0 = adapter_of(K, N, T, r)
    B = B0 if B is None else B
    lib = hip.lib()
    ref = fresh_output(mode, c, M, N)
    ws16 = scratch(int(lib.vlr_gemv_lora_workspace_bytes(16, N, K, T * r)))
    u16 = scratch(int(lib.vlr_gemv_lora_u_bytes(16, K, T * r)))
    for m0 in range(0, M, 16):
        gemv(hip, "vlr_gemv_w4_lora", mode, c, ref, m0, min(16, M - m0), N, K, ws16, (A, B, r, T, outs, 0.25, u16), rope)
    Y = fresh_output(mode, c, M, N)
    ws = scratch(int(lib.vlr_gemv_wide_lora_workspace_bytes(M, N, K, T * r)))
    u = scratch(int(lib.vlr_gemv_wide_lora_u_bytes(M, K, T * r)))
    gemv(hip, "vlr_gemv_wide_w4_lora", mode, c, Y, 0, M, N, K, ws, (A, B, r, T, outs, 0.25, u), rope)
    torch.cuda.synchronize()
    return Y, ref, ws, u


# (mode, targets, pass the row split): q|k|v in three unequal blocks under RoPE, two unequal blocks, gate|up (equal halves, the split left
# to the library), one target on the fp32 stream
LORA_FORMS = [(ROPE, 3, True), (BF16, 2, True), (SWIGLU, 2, False), (F32RES, 1, False)]


@pytest.mark.parametrize("N,K,g", [(136, 416, 32), (256, 8192, 128)])
@pytest.mark.parametrize("r", [8, 72])
@pytest.mark.parametrize("mode,T,split", LORA_FORMS)
def test_wide_w4_lora_equals_16_row_groups(hip, mode, T, split, r, N, K, g):
    """the live adapter over the packed base: x A^T through the wide bf16 kernel, the adapter slice over the row tiles of a 128-column
    block (target edges fall inside it); B = 0 and a NULL adapter give the adapter-free bits"""
    c = inputs(N, K, g)
    outs = (hip.C.c_int * T)(*lora_outs(T, N)) if split else None
    for M in (17, 33, 64):
        Y, ref, ws, u = lora_pair(hip, mode, c, M, N, K, T, r, outs)
        check_rows(Y, ref, M, f"mode {mode} targets {T} r {r} N {N} K {K} M {M}")
    M = 33
    plain, zero, null = (fresh_output(mode, c, M, N) for _ in range(3))
    A, B = adapter_of(K, N, T, r)
    gemv(hip, "vlr_gemv_wide_w4", mode, c, plain, 0, M, N, K, ws)
    gemv(hip, "vlr_gemv_wide_w4_lora", mode, c, zero, 0, M, N, K, ws, (A, torch.zeros_like(B), r, T, outs, 0.25, u))
    gemv(hip, "vlr_gemv_wide_w4_lora", mode, c, null, 0, M, N, K, ws, (None, None, r, T, outs, 0.25, u))
    torch.cuda.synchronize()
    assert not torch.equal(Y[:M], plain[:M]), "the adapter changes the result"
    check_rows(zero, plain, M, "B = 0")
    check_rows(null, plain, M, "NULL adapter")


@pytest.mark.parametrize("M", [20, 49])
def test_wide_w4_lora_one_adapter_over_fused_qkv_and_down_with_residual(hip, M):
    """the adapter layout of a fused q|k|v checkpoint (qkv_targets = 1) at grouped-query widths - heads 2, kv_heads 1, head_dim 128: ONE
    adapter over the 512 fused rows under RoPE (q and k rotated, v plain) - and a `down` adapter added to the fp32 residual stream"""
    H, I, hd = 256, 512, 128
    N = 4 * hd
    c = inputs(N, H, 32)
    Y, ref, _, _ = lora_pair(hip, ROPE, c, M, N, H, 1, 16, None, rope=(hd, 3 * hd))
    check_rows(Y, ref, M, f"fused q|k|v, one adapter, M {M}")
    c = inputs(H, I, 128)
    Y, ref, _, _ = lora_pair(hip, F32RES, c, M, H, I, 1, 16, None)
    check_rows(Y, ref, M, f"down + fp32 residual, M {M}")


def test_argument_errors_and_size_helpers(hip):
    """M = 0 and M = 65 are VLR_ERR_ARG with the row rule in the text and launch nothing; the 16-row entry points keep their own rule;
    the wide size is the 16-row one up to 16 rows and M x the per-row size above"""
    N, K, g, r = 136, 416, 32, 8
    c = inputs(N, K, g)
    A, B = adapter_of(K, N, 1, r)
    lib = hip.lib()
    ws = scratch(int(lib.vlr_gemv_wide_lora_workspace_bytes(64, N, K, r)))
    u = scratch(int(lib.vlr_gemv_wide_lora_u_bytes(64, K, r)))
    Y = torch.full((MMAX + 3, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    for M in (0, 65):
        with pytest.raises(ValueError, match="vlr_gemv_wide_w4: .*1 <= M <= 64"):
            gemv(hip, "vlr_gemv_wide_w4", BF16, c, Y, 0, M, N, K, ws)
        with pytest.raises(ValueError, match="vlr_gemv_wide_w4_lora: .*1 <= M <= 64"):
            gemv(hip, "vlr_gemv_wide_w4_lora", BF16, c, Y, 0, M, N, K, ws, (A, B, r, 1, None, 1.0, u))
    with pytest.raises(ValueError, match="1 <= M <= 16"):
        gemv(hip, "vlr_gemv_w4", BF16, c, Y, 0, 17, N, K, ws)
    with pytest.raises(ValueError, match="1 <= M <= 16"):
        gemv(hip, "vlr_gemv_w4_lora", BF16, c, Y, 0, 17, N, K, ws, (A, B, r, 1, None, 1.0, u))
    torch.cuda.synchronize()
    assert torch.isnan(Y.float()).all()
    for N, K, _ in SHAPES:
        for M in (1, 16):
            assert lib.vlr_gemv_wide_w4_workspace_bytes(M, N, K) == lib.vlr_gemv_w4_workspace_bytes(M, N, K) > 0
        assert lib.vlr_gemv_wide_w4_workspace_bytes(49, N, K) == 49 * lib.vlr_gemv_w4_workspace_bytes(1, N, K)
        assert lib.vlr_gemv_wide_w4_workspace_bytes(200, N, K) == lib.vlr_gemv_wide_w4_workspace_bytes(64, N, K)


# ---- the packed decoder layer at batch 33: 64-row groups (wide scratch) against the 16-row groups (scratch sized for 16 rows)
_LAYERS = {}


def layer_case(hip, qkv_targets):
    """heads 2, kv_heads 1, head_dim 128 (grouped-query), hidden 256, inter 512, group 32; adapters of rank 16 on all four projections"""
    if qkv_targets in _LAYERS:
        return _LAYERS[qkv_targets]
    H, I, nh, nkv, hd, max_pos, B, S, r, g = 256, 512, 2, 1, 128, 512, 33, 20, 16, 32
    Nq, Nkv = nh * hd, nkv * hd
    N = Nq + 2 * Nkv
    cos = torch.empty(max_pos, hd // 2, dtype=torch.float32, device=DEV)
    sin = torch.empty_like(cos)
    hip.call("vlr_rope_table", cos, sin, max_pos, hd, 10000.0)
    sc = 1.0 / math.sqrt(H)
    dense = dict(qkv=rnd(N, H, scale=sc, seed=21), o=rnd(H, Nq, scale=sc, seed=22), gu=rnd(2 * I, H, scale=sc, seed=24),
                 down=rnd(H, I, scale=1 / math.sqrt(I), seed=25))
    packed = {k: {n: t.to(DEV) for n, t in R.pack(*R.quantize_rtn(w.cpu(), g), g).items()} for k, w in dense.items()}
    W = dict(ln1=(1 + 0.1 * rnd(H, seed=20).float()).bfloat16(), ln2=(1 + 0.1 * rnd(H, seed=23).float()).bfloat16(), bqkv=rnd(N, scale=0.1, seed=26))
    Ad = dict(a_qkv=rnd(qkv_targets * r, H, scale=sc, seed=30), b_qkv=rnd(N, r, scale=0.3, seed=31), a_o=rnd(r, Nq, scale=sc, seed=32),
              b_o=rnd(H, r, scale=0.3, seed=33), a_gu=rnd(2 * r, H, scale=sc, seed=34), b_gu=rnd(2 * I, r, scale=0.3, seed=35),
              a_down=rnd(r, I, scale=1 / math.sqrt(I), seed=36), b_down=rnd(H, r, scale=0.3, seed=37))
    cap = S + 4
    km = torch.zeros(B, cap, dtype=torch.int32, device=DEV)
    km[:, :S + 1] = 1
    for b in range(B):
        km[b, :b % 7] = 0                                     # left padding of unequal lengths
    c = dict(H=H, I=I, nh=nh, nkv=nkv, hd=hd, B=B, S=S, r=r, g=g, cap=cap, Nq=Nq, N=N, W=W, packed=packed, Ad=Ad, cos=cos, sin=sin, km=km,
             max_pos=max_pos, qkv_targets=qkv_targets, pos=(km[:, :S].sum(1)).to(torch.int32).contiguous(),
             kc=rnd(B, nkv, cap, hd, seed=40), vc=rnd(B, nkv, cap, hd, seed=41), x=rnd(B, H, seed=42, dtype=torch.float32))
    _LAYERS[qkv_targets] = c
    return c


def run_layer(hip, c, resid_f32, lora, wide):
    """one decode step of the packed layer at column S -> (x_inout, the K column, the V column written)"""
    H, I, nh, nkv, B, N, Nq, r = (c[k] for k in ("H", "I", "nh", "nkv", "B", "N", "Nq", "r"))
    lib = hip.lib()
    cfg = hip.LlamaCfg(H, I, nh, c["hd"], 1e-5, c["max_pos"], c["cos"].data_ptr(), c["sin"].data_ptr(), nkv, resid_f32)
    lw = hip.LayerWeights(c["W"]["ln1"].data_ptr(), None, None, c["W"]["ln2"].data_ptr(), None, None, c["W"]["bqkv"].data_ptr())
    q4 = hip.LayerWeightsW4(*(hip.W4Linear(p["qweight"].data_ptr(), p["qzeros"].data_ptr(), p["scales"].data_ptr(), c["g"])
                              for p in (c["packed"][k] for k in ("qkv", "o", "gu", "down"))))
    shapes, rt = ((N, H), (H, Nq), (2 * I, H), (H, I)), (c["qkv_targets"] * r, r, 2 * r, r)
    mb = min(B, 64) if wide else 16
    if lora:
        fw, fu = (lib.vlr_gemv_wide_lora_workspace_bytes, lib.vlr_gemv_wide_lora_u_bytes) if wide else \
            (lib.vlr_gemv_lora_workspace_bytes, lib.vlr_gemv_lora_u_bytes)
        gb = max(int(fw(mb, n, k, t)) for (n, k), t in zip(shapes, rt))
        ub = max(int(fu(mb, k, t)) for (n, k), t in zip(shapes, rt))
    else:
        fw = lib.vlr_gemv_wide_w4_workspace_bytes if wide else lib.vlr_gemv_w4_workspace_bytes
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
                             c["qkv_targets"], None)
        hip.call("vlr_decoder_layer_decode_w4_lora", cfg, lw, q4, lo, dws, lws, x, c["pos"], kc, vc, c["km"], B, c["cap"], c["S"])
    else:
        hip.call("vlr_decoder_layer_decode_w4", cfg, lw, q4, dws, x, c["pos"], kc, vc, c["km"], B, c["cap"], c["S"])
    torch.cuda.synchronize()
    assert torch.isnan(kc[:, :, c["S"] + 1:].float()).all()
    return x, kc[:, :, c["S"]].clone(), vc[:, :, c["S"]].clone()


@pytest.mark.parametrize("lora,qkv_targets", [(False, 3), (True, 3), (True, 1)])
@pytest.mark.parametrize("resid_f32", [0, 1])
def test_packed_decoder_layer_wide_scratch_equals_16_row_groups(hip, resid_f32, lora, qkv_targets):
    c = layer_case(hip, qkv_targets)
    xw, kw, vw = run_layer(hip, c, resid_f32, lora, wide=True)
    xg, kg, vg = run_layer(hip, c, resid_f32, lora, wide=False)
    assert torch.isfinite(xw.float()).all() and torch.isfinite(kw.float()).all() and torch.isfinite(vw.float()).all()
    assert not torch.equal(xw.float(), c["x"]), "the layer moved the stream"
    same_bits(xw, xg, "x_inout")
    same_bits(kw, kg, "the new K column")
    same_bits(vw, vg, "the new V column")
