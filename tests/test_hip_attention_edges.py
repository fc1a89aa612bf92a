"""Attention kernels (csrc/attention.hip, csrc/decode.hip) at the masks, lengths, head groups and score ranges the product reaches,
against the fp64 reference of tests/attn_ref.py with the per-tile checker (error per (sequence, head, 64-row tile), exact zeros and
lse = +inf where a row sees no key).  Tolerances: attn_ref.TOL, set from the kernels' rounding model (tests/test_attn_checker_host.py).
Every output buffer and the delta workspace start as NaN.  Needs a real MI355X:  pytest -m gpu"""
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import attn_ref as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return _hip


def _nan(*shape, dtype=torch.bfloat16):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _qkv(q, k, v):
    B, S = q.shape[:2]
    return torch.cat([q.reshape(B * S, -1), k.reshape(B * S, -1), v.reshape(B * S, -1)], 1).to(DEV).contiguous()


def run_attention(hip, c, qkv, do, km):
    """forward (and backward when do is given) of case c through vlr_attn_fwd_gqa / vlr_attn_bwd_gqa -> Attn (o, token-major lse,
    dq, dk, dv); checks the padded rows of lse (+inf) and of the delta workspace (0)"""
    B, S, nh, nkv, D = c.B, c.S, c.nh, c.nkv, c.D
    Hq, Hkv = nh * D, nkv * D
    N = Hq + 2 * Hkv
    Sp = (S + 63) // 64 * 64
    scale = 1.0 / math.sqrt(D)
    o = _nan(B * S, Hq)
    lse = _nan(B, nh, Sp, dtype=torch.float32)
    hip.call("vlr_attn_fwd_gqa", qkv, qkv[:, Hq:], qkv[:, Hq + Hkv:], N, o, Hq, lse, km, B, S, nh, nkv, D, int(c.causal), scale)
    dq = dk = dv = None
    if do is not None:
        dqkv = _nan(B * S, N)
        delta = _nan(B, nh, Sp, dtype=torch.float32)
        hip.call("vlr_attn_bwd_gqa", qkv, qkv[:, Hq:], qkv[:, Hq + Hkv:], N, o, do, Hq, lse, delta, km, dqkv, dqkv[:, Hq:],
                 dqkv[:, Hq + Hkv:], N, B, S, nh, nkv, D, int(c.causal), scale)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(delta).all()) and float(delta[:, :, S:].abs().max() if Sp > S else 0.0) == 0.0
        dq = dqkv[:, :Hq].reshape(B, S, nh, D)
        dk = dqkv[:, Hq:Hq + Hkv].reshape(B, S, nkv, D)
        dv = dqkv[:, Hq + Hkv:].reshape(B, S, nkv, D)
    torch.cuda.synchronize()
    assert bool((lse[:, :, S:] == math.inf).all())
    return A.Attn(o.reshape(B, S, nh, D), lse[:, :, :S].transpose(1, 2), dq, dk, dv, None, None, None)


CASES = A.cases()


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_attention_parity(hip, c):
    q, k, v, do, km = A.make_inputs(c, seed=1)
    kmd = None if km is None else km.to(DEV)
    dod = None if do is None else do.reshape(c.B * c.S, -1).to(DEV).contiguous()
    res = run_attention(hip, c, _qkv(q, k, v), dod, kmd)
    ref = A.ref_attention(q.to(DEV), k.to(DEV), v.to(DEV), kmd, c.causal, do=None if do is None else do.to(DEV), o_bwd=res.o)
    worst = A.check_attention(res, ref, A.TOL[c.group], c.name, fwd_only=do is None)
    print(c.name, " ".join(f"{n}={e:.2e}" for n, e in worst.items()))


# ---------------------------------------------------------------------------------------------------- persistent forward, streams
def _persistent_inputs(i):
    B, S, nh, D = 4, 2048, 16, 128          # 8 XCDs x 8 K/V-head slots x 16 blocks = 1024 workgroups > 2 per CU: the persistent path
    g = torch.Generator().manual_seed(100 + i)
    qkv = torch.randn(B * S, 3 * nh * D, generator=g).to(torch.bfloat16).to(DEV)
    km = torch.ones(B, S, dtype=torch.int32)
    km[i % B, :37 * (i + 1)] = 0
    return qkv, km.to(DEV)


@pytest.mark.parametrize("nstreams", [2, 9])
def test_persistent_forward_on_concurrent_streams(hip, nstreams):
    """the persistent forward keeps its ticket counters per stream (8 slots, then the one-workgroup-per-block grid): forwards on
    nstreams streams at once, issued without a synchronisation in between, twice, are bit-identical to each run alone"""
    B, S, nh, D = 4, 2048, 16, 128
    H = nh * D
    scale = 1.0 / math.sqrt(D)
    inputs = [_persistent_inputs(i) for i in range(nstreams)]

    def fwd(qkv, km, o, lse):
        hip.call("vlr_attn_fwd", qkv, qkv[:, H:], qkv[:, 2 * H:], 3 * H, o, H, lse, km, B, S, nh, D, 1, scale)

    alone = []
    for qkv, km in inputs:
        o, lse = _nan(B * S, H), _nan(B, nh, S, dtype=torch.float32)
        fwd(qkv, km, o, lse)
        torch.cuda.synchronize()
        alone.append((o, lse))
    streams = [torch.cuda.Stream() for _ in range(nstreams)]
    outs = [[(_nan(B * S, H), _nan(B, nh, S, dtype=torch.float32)) for _ in range(nstreams)] for _ in range(2)]
    torch.cuda.synchronize()
    for rep in range(2):
        for i, st in enumerate(streams):
            with torch.cuda.stream(st):
                fwd(*inputs[i], *outs[rep][i])
    torch.cuda.synchronize()
    for rep in range(2):
        for i in range(nstreams):
            assert torch.equal(outs[rep][i][0].view(torch.int16), alone[i][0].view(torch.int16)), (rep, i)
            assert torch.equal(outs[rep][i][1], alone[i][1]), (rep, i)
    # and one of them against the reference (the persistent schedule computes the right thing, not only the same thing)
    qkv, km = inputs[1]
    q, k, v = (qkv[:, j * H:(j + 1) * H].reshape(B, S, nh, D) for j in range(3))
    ref = A.ref_attention(q[:1], k[:1], v[:1], km[:1], True)
    c = A._case("masks", 1, S, nh=nh)
    res = A.Attn(alone[1][0].reshape(B, S, nh, D)[:1], alone[1][1][:1].transpose(1, 2), None, None, None, None, None, None)
    A.check_attention(res, ref, A.TOL[c.group], "persistent forward", fwd_only=True)


# ---------------------------------------------------------------------------------------------------- register-staged kernels
def test_register_staged_kernels_in_child_process():
    """VLR_ATTN_DMA=0 (read once per process) routes multi-head attention to the kernels that S > 8192 takes by default
    (attn_fwd_kernel, attn_bwd_dq_kernel, attn_bwd_dkv_kernel): the mask, length and score-range cases of this file on them"""
    env = dict(os.environ, VLR_ATTN_DMA="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_hip_attention_edges.py"), "-q", "-x", "-m", "gpu",
                        "-p", "no:cacheprovider", "-k", "parity and (masks or lengths or scores)"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-1000:]


# ---------------------------------------------------------------------------------------------------- decode attention
DECODE = [  # (name, B, nh, nkv, L, pads per sequence, scores)
    ("pads", 5, 16, 4, 700, (0, 63, 64, 300, 699), "normal"),
    ("group8-pads", 5, 16, 2, 700, (0, 63, 64, 300, 699), "normal"),
    ("group8", 2, 32, 4, 300, (0, 5), "normal"),
    ("len64", 2, 32, 8, 64, (0, 63), "normal"),
    ("len65", 2, 32, 8, 65, (0, 64), "normal"),
    ("len256", 2, 32, 8, 256, (0, 128), "normal"),
    ("len257", 2, 32, 8, 257, (0, 256), "normal"),
    ("C256", 4, 32, 32, 2000, (0, 700, 1999, 3), "normal"),      # 4 x 32 x ceil(2000 / 256) >= 1024 workgroups: 256-key chunks
    ("sink", 3, 16, 4, 700, (0, 64, 300), "sink"),
    ("spike", 3, 16, 4, 700, (0, 64, 300), "spike"),
]


@pytest.mark.parametrize("name,B,nh,nkv,L,pads,scores", DECODE, ids=[d[0] for d in DECODE])
def test_decode_attention_edges(hip, name, B, nh, nkv, L, pads, scores):
    """vlr_attn_decode_gqa (one query row against a cache of L keys) against the fp64 reference, per (sequence, head) at the per-tile
    tolerance, with left padding that masks whole key chunks (the combine kernel's m = -inf skip); two calls are bit-identical"""
    D = 128
    cap = L + 5
    g = torch.Generator().manual_seed(7)
    q = torch.randn(B, nh, D, generator=g)
    kc = torch.randn(B, nkv, cap, D, generator=g)
    vc = torch.randn(B, nkv, cap, D, generator=g)
    km = torch.zeros(B, cap, dtype=torch.int32)
    for b in range(B):
        km[b, pads[b]:L] = 1
    u = torch.randn(D, generator=g)
    u = u / u.norm()
    if scores != "normal":
        q = q + 4.0 * u                                          # q . u ~ 4: a key + 10 sqrt(D) u scores ~40 above the rest
        for b in range(B):
            j = pads[b] if scores == "sink" else L - 1
            kc[b, :, j] += 10.0 * math.sqrt(D) * u
    q, kc, vc = q.to(torch.bfloat16), kc.to(torch.bfloat16), vc.to(torch.bfloat16)
    scale = 1.0 / math.sqrt(D)
    ws = torch.empty(int(hip.lib().vlr_attn_decode_workspace_bytes(B, nh, cap)), dtype=torch.uint8, device=DEV)
    qd, kd, vd, kmd = q.reshape(B, nh * D).to(DEV), kc.to(DEV), vc.to(DEV), km.to(DEV)
    outs = []
    for _ in range(2):
        od = _nan(B, nh * D)
        hip.call("vlr_attn_decode_gqa", qd, nh * D, kd, vd, kmd, od, nh * D, ws, B, nh, nkv, D, cap, L, scale)
        outs.append(od)
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    ref = torch.empty(B, nh, D, dtype=torch.float64, device=DEV)
    G = nh // nkv
    for b in range(B):
        for h in range(nh):
            s = (kd[b, h // G, :L].double() @ qd[b, h * D:(h + 1) * D].double()) * scale
            s = s.masked_fill(kmd[b, :L] == 0, -math.inf)
            ref[b, h] = torch.softmax(s, 0) @ vd[b, h // G, :L].double()
    A.check_tiles(outs[0].reshape(B, 1, nh, D), ref.reshape(B, 1, nh, D), A.TOL["masks"]["o"], rows=1, what=f"decode {name}")
