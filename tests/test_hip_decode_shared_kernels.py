"""Decode attention over a SHARED prompt cache (csrc/decode.hip: attn_shared_prompt_kernel + the tail + one fold) and the decode layer
on it, through the C ABI on the MI355X: against fp32 eager attention and against the per-sequence kernels on the materialised caches
(every sample's prompt columns repeated in front of its tail).  Outputs and every cache column that is not open are NaN-poisoned before
each call.  Needs a real MI355X:  pytest -m gpu"""
import math

import pytest
import torch

from tests import gptq_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
HD = 128


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
    print(f"  {what}: max-relative error {e:.3e} (bound {tol:.1e})")
    assert math.isfinite(e) and e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"


def nan_like(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def prompt_mask(P, Lp):
    """every prompt but the first is left-padded; at prompt_len 321 the last prompt has its first 300 columns masked (whole chunks at
    every chunk size the kernel picks)"""
    km = torch.ones(P, Lp, dtype=torch.int32, device=DEV)
    for p in range(1, P):
        km[p, :min(Lp - 1, 7 * p)] = 0
    if P > 1 and Lp > 320:
        km[P - 1, :300] = 0
    return km


def kv_struct(hip, kp, vp, kmp, P, cap_p, Lp, kt, vt, n, cap_t, Lt):
    return hip.KvShared(kp.data_ptr(), vp.data_ptr(), kmp.data_ptr(), P, cap_p, Lp, kt.data_ptr(), vt.data_ptr(), n, cap_t, Lt)


# (heads, kv_heads, prompts, fanout, prompt_len, tail_len): every value of every axis of the grid; fanout 17 at G = 1 and fanout 5 at
# G = 4 cross a 16-row tile edge; prompt_len 321 with several prompts masks whole chunks.  The last case is the one size at which the
# prompt kernel takes its 128-key chunk (prompts * kv_heads * ceil(prompt_len / 128) >= 1024 workgroups), again with two chunks masked.
ATTN_CASES = [
    (32, 32, 1, 17, 63, 1),
    (32, 8, 3, 5, 321, 70),
    (2, 1, 3, 1, 1, 2),
    (32, 32, 3, 2, 64, 70),
    (32, 8, 1, 16, 64, 2),
    (2, 1, 1, 16, 321, 1),
    (2, 1, 3, 17, 63, 2),
    (32, 8, 3, 2, 1, 1),
    (32, 32, 3, 5, 321, 2),
    (32, 32, 3, 2, 1400, 2),
]


@pytest.mark.parametrize("nh,nkv,P,n,Lp,Lt", ATTN_CASES)
def test_attn_decode_shared_matches_eager_and_materialised(hip, nh, nkv, P, n, Lp, Lt):
    """vlr_attn_decode_shared == fp32 eager softmax attention over [prompt | tail] (1.2e-2, the bound of the per-sequence kernel's test)
    and == vlr_attn_decode_gqa on the materialised cache (1.6e-2, that test's bound between two kernels); two calls bit-identical; NaN
    in every column beyond prompt_len / tail_len does not reach the output"""
    Hq, Hkv = nh * HD, nkv * HD
    N = Hq + 2 * Hkv
    B = P * n
    cap_p, cap_t = Lp + 5, Lt + 3
    rows_p = rnd(P * Lp, N, seed=31)                        # the prompts' q|k|v rows (q unused)
    rows_t = rnd(B * Lt, N, seed=32)                        # every sample's own rows; the query is its last one
    kmp = torch.zeros(P, cap_p, dtype=torch.int32, device=DEV)
    kmp[:, :Lp] = prompt_mask(P, Lp)
    kp, vp = nan_like((P, nkv, cap_p, HD), torch.bfloat16), nan_like((P, nkv, cap_p, HD), torch.bfloat16)
    hip.call("vlr_kv_cache_write", rows_p[:, Hq:], rows_p[:, Hq + Hkv:], N, kp, vp, P, Lp, nkv, HD, cap_p, 0)
    kt, vt = nan_like((B, nkv, cap_t, HD), torch.bfloat16), nan_like((B, nkv, cap_t, HD), torch.bfloat16)
    hip.call("vlr_kv_cache_write", rows_t[:, Hq:], rows_t[:, Hq + Hkv:], N, kt, vt, B, Lt, nkv, HD, cap_t, 0)
    q = rows_t.view(B, Lt, N)[:, Lt - 1].contiguous()
    scale = 1.0 / math.sqrt(HD)
    kv = kv_struct(hip, kp, vp, kmp, P, cap_p, Lp, kt, vt, n, cap_t, Lt)
    wb = int(hip.lib().vlr_attn_decode_shared_workspace_bytes(P, n, nh, cap_p, cap_t))
    assert wb > 0
    ws = torch.full((wb // 4,), float("nan"), dtype=torch.float32, device=DEV)
    o1 = nan_like((B, Hq), torch.bfloat16)
    hip.call("vlr_attn_decode_shared", q, N, kv, o1, Hq, ws, nh, nkv, HD, scale)
    o2 = nan_like((B, Hq), torch.bfloat16)
    hip.call("vlr_attn_decode_shared", q, N, kv, o2, Hq, ws, nh, nkv, HD, scale)
    # the materialised cache of every sample: its prompt's columns, then its tail
    L = Lp + Lt
    cap = L + 9
    kc, vc = nan_like((B, nkv, cap, HD), torch.bfloat16), nan_like((B, nkv, cap, HD), torch.bfloat16)
    kc[:, :, :Lp], vc[:, :, :Lp] = kp[:, :, :Lp].repeat_interleave(n, 0), vp[:, :, :Lp].repeat_interleave(n, 0)
    kc[:, :, Lp:L], vc[:, :, Lp:L] = kt[:, :, :Lt], vt[:, :, :Lt]
    kmc = torch.zeros(B, cap, dtype=torch.int32, device=DEV)
    kmc[:, :Lp] = kmp[:, :Lp].repeat_interleave(n, 0)
    kmc[:, Lp:L] = 1
    wsg = torch.empty(int(hip.lib().vlr_attn_decode_workspace_bytes(B, nh, cap)), dtype=torch.uint8, device=DEV)
    og = nan_like((B, Hq), torch.bfloat16)
    hip.call("vlr_attn_decode_gqa", q, N, kc, vc, kmc, og, Hq, wsg, B, nh, nkv, HD, cap, L, scale)
    torch.cuda.synchronize()
    G = nh // nkv
    qf = q.float()[:, :Hq].reshape(B, nh, 1, HD)
    kf = kc[:, :, :L].float().repeat_interleave(G, dim=1)
    vf = vc[:, :, :L].float().repeat_interleave(G, dim=1)
    s = (qf @ kf.transpose(-1, -2)) * scale
    s = s.masked_fill(kmc[:, None, None, :L] == 0, float("-inf"))
    ref = (s.softmax(-1) @ vf).reshape(B, Hq)
    check(o1, ref, 1.2e-2, "shared vs fp32 eager")
    check(o1, og.float(), 1.6e-2, "shared vs vlr_attn_decode_gqa on the materialised cache")
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16))
    # nothing was written beyond the open columns
    assert bool(torch.isnan(kp[:, :, Lp:].float()).all()) and bool(torch.isnan(kt[:, :, Lt:].float()).all())


def test_attn_decode_shared_argument_errors(hip):
    """every rule is checked before a launch: the output stays poisoned"""
    nh, nkv, P, n, Lp, Lt = 2, 1, 1, 2, 4, 1
    B, Hq = P * n, nh * HD
    kp = rnd(P, nkv, Lp + 2, HD, seed=1)
    kt = rnd(B, nkv, Lt + 2, HD, seed=2)
    km = torch.ones(P, Lp + 2, dtype=torch.int32, device=DEV)
    q = rnd(B, Hq, seed=3)
    o = nan_like((B, Hq), torch.bfloat16)
    ws = torch.empty(int(hip.lib().vlr_attn_decode_shared_workspace_bytes(P, n, nh, Lp + 2, Lt + 2)), dtype=torch.uint8, device=DEV)

    def call(heads=nh, kvh=nkv, hd=HD, **over):
        f = dict(P=P, cap_p=Lp + 2, Lp=Lp, n=n, cap_t=Lt + 2, Lt=Lt)
        f.update(over)
        kv = kv_struct(hip, kp, kp, km, f["P"], f["cap_p"], f["Lp"], kt, kt, f["n"], f["cap_t"], f["Lt"])
        hip.call("vlr_attn_decode_shared", q, Hq, kv, o, Hq, ws, heads, kvh, hd, 0.1)

    for kw, msg in ((dict(hd=64), "head_dim"), (dict(heads=3, kvh=2), "multiple of kv_heads"), (dict(Lp=0), "prompt_len"),
                    (dict(Lp=Lp + 3), "prompt_len"), (dict(Lt=0), "tail_len"), (dict(Lt=Lt + 3), "tail_len"), (dict(n=0), "fanout")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    with pytest.raises(ValueError, match="null"):
        hip.call("vlr_attn_decode_shared", q, Hq, None, o, Hq, ws, nh, nkv, HD, 0.1)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o.float()).all())


# ---------------------------------------------------------------------------------------------------- the decode layer on the shared cache
def layer_case(hip, H, I, nh, nkv, resid_f32, P=2, n=3, Lp=40, Lt=2):
    """weights, a random shared cache (prompt columns and the tails' earlier columns), its materialised form and the scratch of both"""
    Nq, Nkv = nh * HD, nkv * HD
    N = Nq + 2 * Nkv
    B = P * n
    max_pos = 4096
    cos = torch.empty(max_pos, HD // 2, dtype=torch.float32, device=DEV)
    sin = torch.empty_like(cos)
    hip.call("vlr_rope_table", cos, sin, max_pos, HD, 10000.0)
    c = dict(H=H, I=I, nh=nh, nkv=nkv, P=P, n=n, B=B, Lp=Lp, Lt=Lt, N=N, Nq=Nq, Nkv=Nkv, cos=cos, sin=sin)
    c["cfg"] = hip.LlamaCfg(H, I, nh, HD, 1e-5, max_pos, cos.data_ptr(), sin.data_ptr(), nkv, resid_f32)
    sc = 1.0 / math.sqrt(H)
    c["W"] = dict(ln1=(1 + 0.1 * rnd(H, seed=20).float()).bfloat16(), wqkv=rnd(N, H, scale=sc, seed=21), wo=rnd(H, Nq, scale=sc, seed=22),
                  ln2=(1 + 0.1 * rnd(H, seed=23).float()).bfloat16(), wgu=rnd(2 * I, H, scale=sc, seed=24),
                  wdown=rnd(H, I, scale=1 / math.sqrt(I), seed=25))
    cap_p, cap_t = Lp + 5, Lt + 3
    kmp = torch.zeros(P, cap_p, dtype=torch.int32, device=DEV)
    kmp[:, :Lp] = prompt_mask(P, Lp)
    kp, vp = nan_like((P, nkv, cap_p, HD), torch.bfloat16), nan_like((P, nkv, cap_p, HD), torch.bfloat16)
    kp[:, :, :Lp], vp[:, :, :Lp] = rnd(P, nkv, Lp, HD, seed=27), rnd(P, nkv, Lp, HD, seed=28)
    kt, vt = nan_like((B, nkv, cap_t, HD), torch.bfloat16), nan_like((B, nkv, cap_t, HD), torch.bfloat16)
    kt[:, :, :Lt - 1], vt[:, :, :Lt - 1] = rnd(B, nkv, Lt - 1, HD, seed=29), rnd(B, nkv, Lt - 1, HD, seed=30)
    L = Lp + Lt                                              # attended columns of the materialised cache, the new one included
    cap = L + 3
    kc, vc = nan_like((B, nkv, cap, HD), torch.bfloat16), nan_like((B, nkv, cap, HD), torch.bfloat16)
    kc[:, :, :Lp], vc[:, :, :Lp] = kp[:, :, :Lp].repeat_interleave(n, 0), vp[:, :, :Lp].repeat_interleave(n, 0)
    kc[:, :, Lp:L - 1], vc[:, :, Lp:L - 1] = kt[:, :, :Lt - 1], vt[:, :, :Lt - 1]
    kmc = torch.zeros(B, cap, dtype=torch.int32, device=DEV)
    kmc[:, :Lp] = kmp[:, :Lp].repeat_interleave(n, 0)
    kmc[:, Lp:L] = 1
    c.update(kmp=kmp, kp=kp, vp=vp, kt=kt, vt=vt, kc=kc, vc=vc, kmc=kmc, cap_p=cap_p, cap_t=cap_t, cap=cap, L=L)
    c["pos"] = (kmc[:, :L].sum(1) - 1).to(torch.int32).contiguous()
    rdt = torch.float32 if resid_f32 else torch.bfloat16
    c["x"] = rnd(B, H, seed=26, dtype=torch.float32).to(rdt)
    return c


def scratch(hip, c, gemv_bytes, attn_bytes, u_bytes=0):
    B, H, I, N, Nq = c["B"], c["H"], c["I"], c["N"], c["Nq"]
    d = dict(xn=torch.empty(B, H, dtype=torch.bfloat16, device=DEV), rstd=torch.empty(B, device=DEV),
             qkv=nan_like((B, N), torch.bfloat16), attn=nan_like((B, Nq), torch.bfloat16),
             act=torch.empty(B, I, dtype=torch.bfloat16, device=DEV), gemv=torch.empty(gemv_bytes, dtype=torch.uint8, device=DEV),
             attn_ws=torch.empty(attn_bytes, dtype=torch.uint8, device=DEV))
    d["struct"] = hip.DecodeWs(d["xn"].data_ptr(), d["rstd"].data_ptr(), d["qkv"].data_ptr(), d["attn"].data_ptr(), d["act"].data_ptr(),
                               d["gemv"].data_ptr(), gemv_bytes, d["attn_ws"].data_ptr(), attn_bytes)
    if u_bytes:
        d["u"] = torch.empty(u_bytes, dtype=torch.uint8, device=DEV)
        d["lora"] = hip.DecodeLoraWs(d["u"].data_ptr(), u_bytes)
    return d


def run_both(hip, c, lw, q4, lora, gemv_bytes, u_bytes, per_sequence):
    """the shared entry and its per-sequence counterpart on the materialised cache -> (x shared, x materialised); asserts the layer bound
    of test_decoder_layer_decode_matches_prefill on the update and bit equality of the new K / V column"""
    l = hip.lib()
    B, nh = c["B"], c["nh"]
    ab_s = int(l.vlr_attn_decode_shared_workspace_bytes(c["P"], c["n"], nh, c["cap_p"], c["cap_t"]))
    ab_m = int(l.vlr_attn_decode_workspace_bytes(B, nh, c["cap"]))
    ds, dm = scratch(hip, c, gemv_bytes, ab_s, u_bytes), scratch(hip, c, gemv_bytes, ab_m, u_bytes)
    kv = kv_struct(hip, c["kp"], c["vp"], c["kmp"], c["P"], c["cap_p"], c["Lp"], c["kt"], c["vt"], c["n"], c["cap_t"], c["Lt"])
    xs, xm = c["x"].clone(), c["x"].clone()
    hip.call("vlr_decoder_layer_decode_shared", c["cfg"], lw, q4, lora, ds["struct"], ds.get("lora"), xs, c["pos"], kv)
    per_sequence(dm, xm)
    torch.cuda.synchronize()
    assert torch.isfinite(xs.float()).all()
    check(xs.float() - c["x"].float(), xm.float() - c["x"].float(), 2e-2, "shared layer update vs per-sequence layer")
    Lt, L = c["Lt"], c["L"]
    assert torch.equal(c["kt"][:, :, Lt - 1].view(torch.int16), c["kc"][:, :, L - 1].view(torch.int16)), "new K column"
    assert torch.equal(c["vt"][:, :, Lt - 1].view(torch.int16), c["vc"][:, :, L - 1].view(torch.int16)), "new V column"
    assert bool(torch.isnan(c["kt"][:, :, Lt:].float()).all()) and bool(torch.isnan(c["kp"][:, :, c["Lp"]:].float()).all())
    # the attention workspace is validated against the shared size
    bad = hip.DecodeWs(ds["xn"].data_ptr(), ds["rstd"].data_ptr(), ds["qkv"].data_ptr(), ds["attn"].data_ptr(), ds["act"].data_ptr(),
                       ds["gemv"].data_ptr(), gemv_bytes, ds["attn_ws"].data_ptr(), ab_s - 4)
    with pytest.raises(ValueError, match="attn_ws"):
        hip.call("vlr_decoder_layer_decode_shared", c["cfg"], lw, q4, lora, bad, ds.get("lora"), xs, c["pos"], kv)


def proj_shapes(c):
    return ((c["N"], c["H"]), (c["H"], c["Nq"]), (2 * c["I"], c["H"]), (c["H"], c["I"]))


@pytest.mark.parametrize("resid_f32", [1, 0])
@pytest.mark.parametrize("H,I,nh,nkv", [(4096, 11008, 32, 32), (256, 256, 2, 1)])
def test_decoder_layer_decode_shared_matches_per_sequence_layer(hip, resid_f32, H, I, nh, nkv):
    c = layer_case(hip, H, I, nh, nkv, resid_f32)
    W = c["W"]
    lw = hip.LayerWeights(*(W[k].data_ptr() for k in ("ln1", "wqkv", "wo", "ln2", "wgu", "wdown")), None)
    gb = max(int(hip.lib().vlr_gemv_workspace_bytes(c["B"], nn, k)) for nn, k in proj_shapes(c))
    run_both(hip, c, lw, None, None, gb, 0, lambda d, x: hip.call(
        "vlr_decoder_layer_decode", c["cfg"], lw, d["struct"], x, c["pos"], c["kc"], c["vc"], c["kmc"], c["B"], c["cap"], c["L"] - 1))


def test_decoder_layer_decode_shared_packed(hip):
    """q4: the packed GPTQ route against vlr_decoder_layer_decode_w4"""
    c = layer_case(hip, 256, 256, 2, 1, 1)
    W, g = c["W"], 32
    packed = {k: {n: t.to(DEV) for n, t in R.pack(*R.quantize_rtn(W[k].cpu(), g), g).items()} for k in ("wqkv", "wo", "wgu", "wdown")}
    lin = lambda k: hip.W4Linear(packed[k]["qweight"].data_ptr(), packed[k]["qzeros"].data_ptr(), packed[k]["scales"].data_ptr(), g)  # noqa: E731
    q4 = hip.LayerWeightsW4(lin("wqkv"), lin("wo"), lin("wgu"), lin("wdown"))
    lw = hip.LayerWeights(W["ln1"].data_ptr(), None, None, W["ln2"].data_ptr(), None, None, None)
    gb = max(int(hip.lib().vlr_gemv_w4_workspace_bytes(c["B"], nn, k)) for nn, k in proj_shapes(c))
    run_both(hip, c, lw, q4, None, gb, 0, lambda d, x: hip.call(
        "vlr_decoder_layer_decode_w4", c["cfg"], lw, q4, d["struct"], x, c["pos"], c["kc"], c["vc"], c["kmc"], c["B"], c["cap"], c["L"] - 1))


def test_decoder_layer_decode_shared_live_adapters(hip):
    """lora (r = 8): the live-adapter route against vlr_decoder_layer_decode_lora"""
    c = layer_case(hip, 256, 256, 2, 1, 1)
    W, r = c["W"], 8
    H, I, N, Nq = c["H"], c["I"], c["N"], c["Nq"]
    A = dict(a_qkv=rnd(3 * r, H, scale=0.05, seed=40), b_qkv=rnd(N, r, scale=0.05, seed=41), a_o=rnd(r, Nq, scale=0.05, seed=42),
             b_o=rnd(H, r, scale=0.05, seed=43), a_gu=rnd(2 * r, H, scale=0.05, seed=44), b_gu=rnd(2 * I, r, scale=0.05, seed=45),
             a_down=rnd(r, I, scale=0.05, seed=46), b_down=rnd(H, r, scale=0.05, seed=47))
    lora = hip.LoraWeights(r, 2.0, 0.0, *(A[k].data_ptr() for k in ("a_qkv", "b_qkv", "a_o", "b_o", "a_gu", "b_gu", "a_down", "b_down")), 3, None)
    lw = hip.LayerWeights(*(W[k].data_ptr() for k in ("ln1", "wqkv", "wo", "ln2", "wgu", "wdown")), None)
    l = hip.lib()
    rt = (3 * r, r, 2 * r, r)
    gb = max(int(l.vlr_gemv_lora_workspace_bytes(c["B"], nn, k, t)) for (nn, k), t in zip(proj_shapes(c), rt))
    ub = max(int(l.vlr_gemv_lora_u_bytes(c["B"], k, t)) for (nn, k), t in zip(proj_shapes(c), rt))
    run_both(hip, c, lw, None, lora, gb, ub, lambda d, x: hip.call(
        "vlr_decoder_layer_decode_lora", c["cfg"], lw, lora, d["struct"], d["lora"], x, c["pos"], c["kc"], c["vc"], c["kmc"], c["B"], c["cap"],
        c["L"] - 1))
