"""The skinny GEMMs with a live LoRA adapter (csrc/decode.hip: vlr_gemv_bf16_lora, vlr_gemv_w4_lora) through the C ABI on the MI355X.
The reference is fp64 on the host from the same bf16 inputs:  x W^T + u B^T  with u = bf16(scale * x A^T), then the mode's epilogue -
the adapter term is in the accumulator BEFORE bias / RoPE / SwiGLU / residual.  The tolerances are those of the adapter-free tests of
the same mode (tests/test_hip_decode_kernels.py, tests/test_hip_gptq.py): 8e-3 bf16 out (plain, residual, RoPE), 1e-5 fp32 residual,
1e-2 SwiGLU.  The adapter's scale is chosen per case so that its term is at least 10 x the tolerance (a missing or mis-blocked term
fails) while the rounding of u moves the reference by less than half of it (both asserted on the host, before the GPU is touched).
Outputs are NaN-poisoned before every call.  Needs a real MI355X:  pytest -m gpu"""
import math

import numpy as np
import pytest
import torch

from tests import gptq_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32RES, ROPE, SWIGLU = 0, 2, 3, 4                      # VLR_GEMV_* modes (include/vlr.h)
TOL = {BF16: 8e-3, F32RES: 1e-5, ROPE: 8e-3, SWIGLU: 1e-2}
HD, MAX_POS = 64, 512                                        # RoPE cases: q 4 heads | k 1 | v 1 (grouped-query: unequal blocks)
QKV = (256, 64, 64)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return _hip


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-12)


def outs_of(mode, N):
    """rows of each fused sub-target: q|k|v unequal (RoPE), gate|up (SwiGLU), one target otherwise"""
    return QKV if mode == ROPE else ((N // 2, N // 2) if mode == SWIGLU else (N,))


def rope_tables():
    inv = 1.0 / (10000.0 ** (torch.arange(0, HD, 2, dtype=torch.float64) / HD))
    ang = torch.arange(MAX_POS, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().float(), ang.sin().float()


def epilogue(mode, acc, c):
    """fp64 epilogue of `mode` on the accumulators acc [M][N]"""
    if mode == SWIGLU:
        I = acc.shape[1] // 2
        g, u = acc[:, :I], acc[:, I:]
        return g * torch.sigmoid(g) * u
    if mode == ROPE:
        acc = acc + c["bias"].double()
        rc = QKV[0] + QKV[1]
        out = acc.clone()
        heads = acc[:, :rc].reshape(acc.shape[0], -1, HD)
        x1, x2 = heads[..., :HD // 2], heads[..., HD // 2:]
        cs, sn = c["cos"][c["pos"].long()].double()[:, None], c["sin"][c["pos"].long()].double()[:, None]
        out[:, :rc] = torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1).reshape(acc.shape[0], rc)
        return out
    return acc + c["res"].double()                           # BF16 with a bf16 residual, F32RES with an fp32 one


def adapter_term(u, B, outs, r):
    """sum_j u[m][t(n) r + j] B[n][j]: row block t of B meets ITS r columns of u"""
    cols, row = [], 0
    for t, o in enumerate(outs):
        cols.append(u[:, t * r:(t + 1) * r] @ B[row:row + o].double().T)
        row += o
    return torch.cat(cols, 1)


_CASES = {}


def case(mode, M, K, N, r, g=None):
    """host inputs and fp64 references of one case, built once and shared.  g: None = bf16 base, else the GPTQ group size (weights from
    tests/gptq_ref.py, the reference W is their dequantised form)"""
    key = (mode, M, K, N, r, g)
    if key in _CASES:
        return _CASES[key]
    seed = 1000 * mode + 97 * M + K + N + r
    outs = outs_of(mode, N)
    T = len(outs)
    c = dict(outs=outs, X=rnd(M, K, seed=seed), A=rnd(T * r, K, scale=0.05, seed=seed + 1), B=rnd(N, r, scale=0.05, seed=seed + 2))
    W = rnd(N, K, scale=0.05, seed=seed + 3)
    if g is not None:
        c["packed"] = R.pack(*R.quantize_rtn(W, g), g)
        W = R.dequant(c["packed"]["qweight"], c["packed"]["qzeros"], c["packed"]["scales"], g)
    c["W"] = W
    if mode == ROPE:
        c["bias"] = rnd(N, seed=seed + 4)
        c["cos"], c["sin"] = rope_tables()
        c["pos"] = torch.tensor([(37 * i + 5) % MAX_POS for i in range(M)], dtype=torch.int32)
    elif mode == BF16:
        c["res"] = rnd(M, N, seed=seed + 4)
    elif mode == F32RES:
        c["res"] = torch.randn(M, N, generator=torch.Generator().manual_seed(seed + 4))
    base = c["X"].double() @ W.double().T
    xa = c["X"].double() @ c["A"].double().T
    c["plain"] = epilogue(mode, base, c)
    # the scale (lora_alpha / r of the call): the adapter term at about 30 x the tolerance of the mode, as an fp32 number
    t1 = adapter_term(xa, c["B"], outs, r)
    c["scale"] = float(np.float32(30 * TOL[mode] * float(c["plain"].abs().max()) / float(t1.abs().max())))
    u_exact = xa * c["scale"]
    u_bf16 = u_exact.float().to(torch.bfloat16).double()    # the kernel's rule: scale in fp32, ONE rounding to bf16
    c["ref"] = epilogue(mode, base + adapter_term(u_bf16, c["B"], outs, r), c)
    c["ref_exact_u"] = epilogue(mode, base + adapter_term(u_exact, c["B"], outs, r), c)
    _CASES[key] = c
    return c


def check_inputs(mode, c):
    """the inputs separate a missing / mis-blocked adapter term from rounding"""
    tol = TOL[mode]
    term = float((c["ref"] - c["plain"]).abs().max()) / float(c["ref"].abs().max())
    assert term >= 10 * tol, f"adapter term {term:.3e} below 10 x tolerance {tol:.1e}"
    e = relerr(c["ref_exact_u"], c["ref"])
    assert e <= tol / 2, f"rounding of u moves the reference by {e:.3e} > half the tolerance {tol:.1e}"


def run(hip, mode, c, M, K, N, r, g=None, adapter=True, B=None, A=None):
    """one call of the _lora entry point (adapter=True) or of the adapter-free one -> the output tensor (bf16, or fp32 under F32RES)"""
    d = lambda t: None if t is None else t.to(DEV)           # noqa: E731
    X = d(c["X"])
    T = len(c["outs"])
    ncols = N // 2 if mode == SWIGLU else N
    if mode == F32RES:
        Y = d(c["res"]).clone()                              # in place on the fp32 residual stream
        res, ldr = Y, N
    else:
        Y = torch.full((M, ncols), float("nan"), dtype=torch.bfloat16, device=DEV)
        res, ldr = (d(c["res"]), N) if mode == BF16 else (None, 0)
    bias = d(c.get("bias"))
    pos, cos, sin = d(c.get("pos")), d(c.get("cos")), d(c.get("sin"))
    rc = QKV[0] + QKV[1] if mode == ROPE else 0
    tail = (Y, ncols, bias, res, ldr, pos, cos, sin, rc, HD, MAX_POS, M, N, K)
    lib = hip.lib()
    if g is None:
        head, fn = (mode, X, K, d(c["W"])), "vlr_gemv_bf16"
        wb = int(lib.vlr_gemv_workspace_bytes(M, N, K))
    else:
        p = c["packed"]
        head, fn = (mode, X, K, d(p["qweight"]), d(p["qzeros"]), d(p["scales"]), R.group(K, g)), "vlr_gemv_w4"
        wb = int(lib.vlr_gemv_w4_workspace_bytes(M, N, K))
    if not adapter:
        ws = torch.empty(wb, dtype=torch.uint8, device=DEV)
        hip.call(fn, *head, *tail, ws)
    else:
        wb = int(lib.vlr_gemv_lora_workspace_bytes(M, N, K, T * r))
        ub = int(lib.vlr_gemv_lora_u_bytes(M, K, T * r))
        assert wb > 0 and ub > 0
        ws = torch.full((wb // 4,), float("nan"), dtype=torch.float32, device=DEV)
        u = torch.full((ub // 4,), float("nan"), dtype=torch.float32, device=DEV)
        outs = (hip.C.c_int * T)(*c["outs"]) if T > 1 else None
        Ad, Bd = (d(c["A"]) if A is None else A), (d(c["B"]) if B is None else B)
        if A == "null":
            Ad = Bd = None
        hip.call(fn + "_lora", *head, *tail, ws, Ad, Bd, r, T, outs, c["scale"], u)
    torch.cuda.synchronize()
    return Y


SHAPES = [(128, 64), (136, 200), (512, 384)]                # K % 128 != 0, N % 64 != 0, several K slices (K = 512: two)


@pytest.mark.parametrize("r", [8, 16, 64])
@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("M", [1, 4, 16])
@pytest.mark.parametrize("mode", [BF16, F32RES, SWIGLU])
def test_gemv_bf16_lora(hip, mode, M, K, N, r):
    """one target (bf16 + residual, fp32 residual in place) and gate|up (two targets, N = 2 I; I = 100 puts the target edge inside a
    column block) against the fp64 host reference; a second call is bit-identical"""
    c = case(mode, M, K, N, r)
    check_inputs(mode, c)
    Y = run(hip, mode, c, M, K, N, r)
    e = relerr(Y, c["ref"])
    print(f"mode {mode} M {M} K {K} N {N} r {r}: rel err {e:.3e} (bound {TOL[mode]:.1e})")
    assert math.isfinite(e) and e <= TOL[mode]
    assert torch.equal(Y, run(hip, mode, c, M, K, N, r)), "two calls in a row"


@pytest.mark.parametrize("r", [8, 16, 64])
@pytest.mark.parametrize("K", [128, 136, 512])
@pytest.mark.parametrize("M", [1, 4, 16])
def test_gemv_bf16_lora_qkv_rope(hip, M, K, r):
    """q 256 | k 64 | v 64 rows (grouped-query: unequal blocks) with a bias and the rotation of the accumulators"""
    N = sum(QKV)
    c = case(ROPE, M, K, N, r)
    check_inputs(ROPE, c)
    Y = run(hip, ROPE, c, M, K, N, r)
    e = relerr(Y, c["ref"])
    print(f"rope M {M} K {K} r {r}: rel err {e:.3e} (bound {TOL[ROPE]:.1e})")
    assert math.isfinite(e) and e <= TOL[ROPE]
    assert torch.equal(Y, run(hip, ROPE, c, M, K, N, r)), "two calls in a row"


@pytest.mark.parametrize("g", [32, -1])
@pytest.mark.parametrize("mode", [BF16, F32RES, ROPE, SWIGLU])
def test_gemv_w4_lora(hip, mode, g):
    """the packed base (GPTQ int4, g = 32: scales per 32-k step; g = -1: one group) with the bf16 adapter slice, every mode"""
    M, K, N, r = 4, 512, 384, 16
    c = case(mode, M, K, N, r, g)
    check_inputs(mode, c)
    Y = run(hip, mode, c, M, K, N, r, g)
    e = relerr(Y, c["ref"])
    print(f"w4 mode {mode} g {g}: rel err {e:.3e} (bound {TOL[mode]:.1e})")
    assert math.isfinite(e) and e <= TOL[mode]
    assert torch.equal(Y, run(hip, mode, c, M, K, N, r, g)), "two calls in a row"


# ranks beyond one LDS chunk of the adapter slice (64-column block: 512 bf16 columns of u per row over the targets it spans; packed,
# 128 columns: 1024): one target in two chunks, a gate|up edge inside a block (2 x 264 -> chunks of 256 + 8), q|k|v at r = 176 and 256
# (3 r > 512; a block spans one target), the packed kernel in two chunks
BIG_RANK = [(BF16, 4, 136, 200, 520, None), (SWIGLU, 16, 136, 200, 264, None), (ROPE, 4, 128, 384, 176, None), (ROPE, 16, 136, 384, 256, None),
            (F32RES, 4, 512, 384, 1032, 32)]


@pytest.mark.parametrize("mode,M,K,N,r,g", BIG_RANK)
def test_rank_beyond_one_lds_chunk(hip, mode, M, K, N, r, g):
    """no rank limit: the slice walks r in chunks, j ascending - against the fp64 reference, B = 0 exact, two calls bit-identical"""
    c = case(mode, M, K, N, r, g)
    check_inputs(mode, c)
    Y = run(hip, mode, c, M, K, N, r, g)
    e = relerr(Y, c["ref"])
    print(f"mode {mode} M {M} K {K} N {N} r {r} g {g}: rel err {e:.3e} (bound {TOL[mode]:.1e})")
    assert math.isfinite(e) and e <= TOL[mode]
    assert torch.equal(Y, run(hip, mode, c, M, K, N, r, g)), "two calls in a row"
    zero = run(hip, mode, c, M, K, N, r, g, B=torch.zeros(N, r, dtype=torch.bfloat16, device=DEV))
    assert torch.equal(zero, run(hip, mode, c, M, K, N, r, g, adapter=False)), "B = 0"


@pytest.mark.parametrize("g", [None, 32])
@pytest.mark.parametrize("mode", [BF16, F32RES, ROPE, SWIGLU])
def test_zero_and_null_adapter_are_exact_no_ops(hip, mode, g):
    """B = 0 (the adapter slice adds 0.0f last) and A = B = NULL: bit-identical to the adapter-free entry point"""
    M, K, N, r = 4, 512, 384, 16
    c = case(mode, M, K, N, r, g)
    plain = run(hip, mode, c, M, K, N, r, g, adapter=False)
    zero = run(hip, mode, c, M, K, N, r, g, B=torch.zeros(N, r, dtype=torch.bfloat16, device=DEV))
    null = run(hip, mode, c, M, K, N, r, g, A="null")
    assert torch.isfinite(plain.float()).all()
    assert torch.equal(plain, zero), "B = 0"
    assert torch.equal(plain, null), "NULL adapter"
    assert not torch.equal(plain, run(hip, mode, c, M, K, N, r, g)), "the live adapter changes the result"


@pytest.mark.parametrize("g", [None, 32])
@pytest.mark.parametrize("target", [0, 1, 2])
def test_only_the_adapted_target_moves(hip, target, g):
    """q|k|v with three different A blocks and a B that is non-zero for ONE target: the other targets' columns equal the adapter-free
    result bit for bit (a row reading another target's u block, or a wrong block edge, would move them), the adapted ones match the
    reference"""
    M, K, r = 4, 512, 16
    N = sum(QKV)
    c = case(ROPE, M, K, N, r, g)
    edges = np.cumsum((0,) + QKV)
    lo, hi = int(edges[target]), int(edges[target + 1])
    B1 = torch.zeros_like(c["B"])
    B1[lo:hi] = c["B"][lo:hi]
    plain = run(hip, ROPE, c, M, K, N, r, g, adapter=False)
    Y = run(hip, ROPE, c, M, K, N, r, g, B=B1.to(DEV))
    keep = torch.ones(N, dtype=torch.bool)
    keep[lo:hi] = False
    assert torch.equal(Y[:, keep], plain[:, keep]), "columns of the targets without an adapter"
    assert not torch.equal(Y[:, lo:hi], plain[:, lo:hi])
    u = ((c["X"].double() @ c["A"].double().T) * c["scale"]).float().to(torch.bfloat16).double()
    acc = c["X"].double() @ c["W"].double().T + adapter_term(u, B1, QKV, r)
    e = relerr(Y, epilogue(ROPE, acc, c))
    assert e <= TOL[ROPE], e


def test_argument_errors_launch_nothing(hip):
    """VLR_ERR_ARG (ValueError through _hip.call) with a vlr_last_error text; the NaN-poisoned output is untouched"""
    M, K, N, r = 4, 128, 64, 8
    c = case(BF16, M, K, N, r)
    X, W, A, B = (c[k].to(DEV) for k in ("X", "W", "A", "B"))
    Y = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    ws = torch.empty(int(hip.lib().vlr_gemv_lora_workspace_bytes(M, N, K, r)), dtype=torch.uint8, device=DEV)
    u = torch.empty(int(hip.lib().vlr_gemv_lora_u_bytes(M, K, r)), dtype=torch.uint8, device=DEV)

    def call(M=M, N=N, K=K, A=A, B=B, r=r, T=1, outs=None, u=u, mode=BF16):
        hip.call("vlr_gemv_bf16_lora", mode, X, K, W, Y, N, None, None, 0, None, None, None, 0, HD, MAX_POS, M, N, K, ws, A, B, r, T, outs, 1.0, u)

    for kw, text in ((dict(r=12), "multiple of 8"), (dict(r=0), "multiple of 8"), (dict(M=17), "1 <= M <= 16"), (dict(M=0), "1 <= M <= 16"),
                     (dict(K=124), "multiple of 8"), (dict(T=0), "targets"), (dict(T=5), "targets"), (dict(T=3), "not a multiple of targets"),
                     (dict(T=2, outs=(hip.C.c_int * 2)(40, 16)), "sum to"), (dict(u=None), "null adapter"), (dict(B=None), "null adapter"),
                     (dict(mode=7), "unknown mode")):
        with pytest.raises(ValueError, match=text):
            call(**kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(Y.float()).all()), "an argument error launched a kernel"
    assert hip.lib().vlr_gemv_lora_workspace_bytes(M, N, K, 12) == 0
