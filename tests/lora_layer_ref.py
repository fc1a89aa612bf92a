"""Cases, float64 reference and bf16 replay of the LoRA decoder-layer passes of csrc/layers.cpp, driven through the C ABI by
tests/test_hip_lora_layer.py and checked on the CPU by tests/test_lora_layer_checker_host.py:

  vlr_decoder_layer_fwd_lora  / _bwd_lora      ("lora":    peft LoRA on every row)
  vlr_decoder_layer_fwd_lora_ex / _bwd_lora_ex ("lora_ex": a row mask - PLoRA - and optionally the base gradients)
  vlr_decoder_layer_fwd_lora2 / _bwd_lora2     ("lora2":   peft LoRA stacked on frozen, row-masked PLoRA)

CASES fixes every argument of one call; branches(case) names the routes of layers.cpp the case takes.
reference(case, inp) is ONE layer written out in float64 torch and differentiated by autograd from a given dy.  The oracle's
llama_hidden computes its RoPE tables, its additive mask and the mean square of rms_norm in float32 whatever dtype it is handed, it
knows neither a row mask nor a q|k|v bias, a fused-projection adapter or a second adapter, and it has no down adapter switch; so the
layer is restated here and llama_hidden serves as a cross-check of this file in the one configuration where it fits
(test_lora_layer_checker_host.py).  The keep mask of target t is oracle.dropout_mask(seed + t) over the FULL [M][in] operand.
replay(case, inp, fault) is the same layer in float32 with a rounding to bf16 wherever the drivers store bf16, the backward written out
call for call in the order of layers.cpp; `fault` plants exactly one wiring error (FAULTS).
Two numbers per tensor: err(T) = max|T - ref| / max|ref| and the least-squares scale c(T) = <T, ref> / <ref, ref>.  The bound of a
tensor is 4 x the replay's err and 4 x the replay's |c - 1| + 2^-9 (half a bf16 ulp of 1) - it never comes from the kernels."""
import math
import zlib

import torch
import torch.nn.functional as F

from oracle import llava_dpo_oracle as O

F64, F32 = torch.float64, torch.float32
HEAD_DIM, HIDDEN, HEADS, INTER = 128, 256, 2, 384
EPS, THETA, MAX_POS, PAD_TAIL = 1e-5, 10000.0, 512, 6
MARGIN, C_FLOOR = 4.0, 2.0 ** -9
GROUPS = ("qkv", "o", "gu", "down")
T0 = dict(qkv=0, o=3, gu=4, down=6)              # first dropout target of a group (seed + t) and its u column block (t * r)
LORA_GRADS = tuple(f"d{m}_{g}" for g in GROUPS for m in "AB")
BASE_GRADS = ("g_ln1", "g_wqkv", "g_wo", "g_ln2", "g_wgu", "g_wdown")


class Case(dict):
    __getattr__ = dict.__getitem__

    @property
    def M(self):
        return self.B * self.S

    @property
    def nq(self):
        return 1 if self.qkv_targets == 1 else 3


def _case(name, family, M, r, p, **kw):
    c = Case(name=name, family=family, B=2, S=M // 2, heads=HEADS, kv_heads=2, hidden=HIDDEN, inter=INTER, r=r, r_p=0, dropout=p,
             dropout_p=0.0, qkv_targets=3, bias=False, down_adapter=True, resid_f32=False, rowmask="none", mask_bits=False,
             mask_bits_p=False, accumulate=0, base_grads=False, scale=2.0, scale_p=1.0)
    c.update(kw)
    assert set(kw) <= set(c) and c.M == M
    assert family != "lora" or (c.rowmask == "none" and not c.base_grads)
    assert family == "lora_ex" or not c.base_grads
    assert (family == "lora2") == (c.r_p > 0)
    return c


CASES = [
    # ---- vlr_decoder_layer_fwd_lora / _bwd_lora
    _case("lora_m140_r8_hash", "lora", 140, 8, 0.25),
    _case("lora_m320_r64_bits_gqa_f32_acc", "lora", 320, 64, 0.25, mask_bits=True, kv_heads=1, down_adapter=False, resid_f32=True,
          accumulate=1),
    _case("lora_m768_r8_p0_fusedqkv_bias_acc", "lora", 768, 8, 0.0, qkv_targets=1, bias=True, accumulate=1),
    _case("lora_m140_r64_bits_gqa_fusedqkv", "lora", 140, 64, 0.25, mask_bits=True, kv_heads=1, qkv_targets=1, resid_f32=True),
    # ---- vlr_decoder_layer_fwd_lora_ex / _bwd_lora_ex
    _case("ex_m140_r8_hash_ragged", "lora_ex", 140, 8, 0.25, rowmask="ragged"),
    _case("ex_m320_r64_bits_edge_gqa_f32_acc_base", "lora_ex", 320, 64, 0.25, rowmask="edge", mask_bits=True, kv_heads=1, resid_f32=True,
          accumulate=1, base_grads=True),
    _case("ex_m768_r64_hash_tile_empty_fusedqkv", "lora_ex", 768, 64, 0.25, rowmask="one_tile_empty", qkv_targets=1, down_adapter=False),
    _case("ex_m320_r8_p0_zero", "lora_ex", 320, 8, 0.0, rowmask="zero"),
    _case("ex_m140_r8_bits_allrows_gqa_base", "lora_ex", 140, 8, 0.25, mask_bits=True, kv_heads=1, base_grads=True, bias=True),
    _case("ex_m768_r64_p0_ragged_base_acc", "lora_ex", 768, 64, 0.0, rowmask="ragged", base_grads=True, accumulate=1),
    _case("ex_m320_r64_bits_ragged", "lora_ex", 320, 64, 0.25, rowmask="ragged", mask_bits=True),
    # ---- vlr_decoder_layer_fwd_lora2 / _bwd_lora2
    _case("two_m140_r8_8_hash_ragged", "lora2", 140, 8, 0.25, r_p=8, dropout_p=0.25, rowmask="ragged"),
    _case("two_m768_r64_256_bits_tile_empty_gqa_f32_acc", "lora2", 768, 64, 0.25, r_p=256, dropout_p=0.25, rowmask="one_tile_empty",
          mask_bits=True, mask_bits_p=True, kv_heads=1, resid_f32=True, accumulate=1),
    _case("two_m320_r64_256_p0_edge_fusedqkv", "lora2", 320, 64, 0.0, r_p=256, rowmask="edge", qkv_targets=1, down_adapter=False),
    _case("two_m320_r8_256_bits_zero_gqa", "lora2", 320, 8, 0.25, r_p=256, rowmask="zero", mask_bits=True, kv_heads=1),
    _case("two_m140_r64_8_allrows_bias", "lora2", 140, 64, 0.0, r_p=8, dropout_p=0.25, bias=True),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---------------------------------------------------------------------------------------------------- routes
def branches(c):
    """the routes of csrc/layers.cpp that the arguments of the case select, as "branch:side" strings"""
    rm = c.rowmask != "none"
    out = {f"qkv_targets:{c.nq}", f"down:{'set' if c.down_adapter else 'null'}", f"resid:{'f32' if c.resid_f32 else 'bf16'}",
           f"accumulate:{c.accumulate}", f"rowmask:{c.rowmask}", f"dropout:{'on' if c.dropout > 0 else 'off'}"}
    if c.nq == 3:
        out.add(f"qkv_widths:{'equal' if c.kv_heads == c.heads else 'unequal'}")       # one grouped launch, or one launch per target
    if c.dropout > 0:
        out.add(f"mask_bits:{'set' if c.mask_bits else 'null'}")                       # streaming row-slab kernels, or the hashing GEMMs
    if c.family == "lora2":
        out.add(f"dropout_p:{'on' if c.dropout_p > 0 else 'off'}")
        if c.dropout_p > 0:
            out.add(f"mask_bits_p:{'set' if c.mask_bits_p else 'null'}")
        if rm:
            out.add(f"tile_skip:{'on' if c.r % 64 == 0 and (c.r + c.r_p) % 64 == 0 else 'off'}")
    else:
        if rm:
            out.add(f"tile_skip:{'on' if c.r % 64 == 0 else 'off'}")                  # r % 64 == 0: the 256-row-tile skip flags
            out.add(f"ktile_list:{'on' if c.M % 64 == 0 else 'off'}")                  # M % 64 == 0: the adapter-gradient K-tile list
    if c.family == "lora_ex":
        out.add(f"base_grads:{'set' if c.base_grads else 'null'}")
    return out


COMMON = {"qkv_targets:1", "qkv_targets:3", "down:set", "down:null", "resid:f32", "resid:bf16", "accumulate:0", "accumulate:1",
          "dropout:on", "dropout:off", "qkv_widths:equal", "qkv_widths:unequal", "mask_bits:set", "mask_bits:null"}
ROWMASKS = {"rowmask:" + k for k in ("none", "ragged", "edge", "one_tile_empty", "zero")}
REQUIRED = {
    "lora": COMMON | {"rowmask:none"},
    "lora_ex": COMMON | ROWMASKS | {"tile_skip:on", "tile_skip:off", "ktile_list:on", "ktile_list:off", "base_grads:set", "base_grads:null"},
    "lora2": COMMON | ROWMASKS | {"tile_skip:on", "tile_skip:off", "dropout_p:on", "dropout_p:off", "mask_bits_p:set", "mask_bits_p:null"},
}


# ---------------------------------------------------------------------------------------------------- inputs
def row_mask(kind, B, S):
    """bool [B * S] (None: every row).  ragged: image rows in two runs per sequence; edge: rows 255, 256 and M - 1 only;
    one_tile_empty: M = 768 with rows 256..511 all text; zero: no image row"""
    M = B * S
    if kind == "none":
        return None
    m = torch.zeros(M, dtype=torch.bool)
    if kind == "ragged":
        for b in range(B):
            for lo, hi in ((3 + 2 * b, S // 4 + b), (S // 2 + 5 * b, S // 2 + S // 3 + 1)):
                m[b * S + lo:b * S + hi] = True
    elif kind == "edge":
        assert M > 257
        m[[255, 256, M - 1]] = True
    elif kind == "one_tile_empty":
        assert M == 768
        m[5:250] = True
        m[255] = True
        m[512] = True
        m[530:700] = True
    else:
        assert kind == "zero"
    return m


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _adapter(g, c, r, scale, p, seed, bits, rows, train):
    H, I, nq = c.hidden, c.inter, c.nq
    Nq, Nkv = c.heads * HEAD_DIM, c.kv_heads * HEAD_DIM
    N = Nq + 2 * Nkv
    b_std = 0.35 / math.sqrt(r)
    a = dict(r=r, scale=scale, p=p, seed=seed, bits=bits, rows=rows, train=train)
    for grp, n, inn, out in (("qkv", nq, H, N), ("o", 1, H, H), ("gu", 2, H, 2 * I), ("down", 1, I, H)):
        if grp == "down" and not c.down_adapter:
            a["A_down"] = a["B_down"] = None
            continue
        a["A_" + grp] = _bf((torch.rand(n * r, inn, generator=g, dtype=F64) * 2 - 1) / math.sqrt(inn) * 1.7)
        a["B_" + grp] = _bf(torch.randn(out, r, generator=g, dtype=F64) * b_std)
    return a


def make(c):
    """every operand of the case in float64, holding the values the device buffers hold (bf16-representable; fp32 for the residual
    stream under resid_f32)"""
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    B, S, M, H, I = c.B, c.S, c.M, c.hidden, c.inter
    Nq, Nkv = c.heads * HEAD_DIM, c.kv_heads * HEAD_DIM
    N = Nq + 2 * Nkv
    rn = lambda *s, std=1.0: torch.randn(*s, generator=g, dtype=F64) * std      # noqa: E731
    inp = dict(ln1=_bf(1 + 0.1 * rn(H)), ln2=_bf(1 + 0.1 * rn(H)), wqkv=_bf(rn(N, H, std=0.05)), wo=_bf(rn(H, H, std=0.05)),
               wgu=_bf(rn(2 * I, H, std=0.05)), wdown=_bf(rn(H, I, std=0.05)), bqkv=_bf(rn(N, std=0.2)) if c.bias else None)
    am = torch.ones(B, S, dtype=torch.long)
    am[1, S - PAD_TAIL:] = 0                                      # row 1 carries a few padded key positions at its end
    inp["key_mask"] = am
    inp["pos"] = (am.cumsum(-1) - 1).masked_fill(am == 0, 1)
    inp["valid"] = am.reshape(-1) != 0
    x = rn(M, H)
    inp["x_in"] = x.float().double() if c.resid_f32 else _bf(x)
    dy = _bf(rn(M, H))
    dy[~inp["valid"]] = 0
    inp["dy"] = dy
    rows = row_mask(c.rowmask, B, S)
    inp["rowmask"] = rows
    seed = 1000003 * (1 + CASES.index(BY_NAME[c.name])) if c.name in BY_NAME else 77
    if c.family == "lora2":
        inp["sets"] = [_adapter(g, c, c.r, c.scale, c.dropout, seed, c.mask_bits, None, True),
                       _adapter(g, c, c.r_p, c.scale_p, c.dropout_p, seed + 5000, c.mask_bits_p, rows, False)]
    else:
        inp["sets"] = [_adapter(g, c, c.r, c.scale, c.dropout, seed, c.mask_bits, rows, True)]
    # the float64 reference, computed once per case and shared; the gradient buffers' contents before the call (read under
    # accumulate = 1 only) are sized to the gradient they receive - a quarter of its largest element - so that a lost or a spurious
    # accumulation moves the result by about its own size while the rounding of old + new stays that of the new gradient
    inp["ref"] = ref = reference(c, inp)
    inp["old"] = {}
    for name in list(LORA_GRADS) + list(BASE_GRADS):
        if name in ref:
            top = float(ref[name].abs().max())
            inp["old"][name] = _bf(rn(*ref[name].shape) * (0.25 * top if top > 0 else 1.0))
    return inp


def keep_mask(a, t, M, inn, fault=None):
    """float keep mask [M][in] of dropout target t of adapter set `a` (None: no dropout): oracle.dropout_mask over the FULL operand"""
    if a["p"] <= 0:
        return None
    if fault == "seed_offset" and t == 3:
        t = 2
    k = O.dropout_mask(a["seed"] + t, M * inn, a["p"]).view(M, inn)
    if fault == "mask_compact_index" and a["rows"] is not None:
        kc = torch.zeros_like(k)
        n = int(a["rows"].sum())
        kc[a["rows"]] = k.reshape(-1)[:n * inn].view(n, inn)     # the mask indexed over the marked rows only
        k = kc
    return k


def packed_bits(a, t, M, inn):
    """the row-major packed keep mask the forward draws for target t: bit e of byte i = element 8 i + e (include/vlr.h)"""
    import numpy as np
    return torch.from_numpy(np.packbits(O.dropout_mask(a["seed"] + t, M * inn, a["p"]).numpy(), bitorder="little"))


def bits_offset(c, t):
    """byte offset of target t's row-major mask inside mask_bits: t < 6 at t * M * hidden / 8, down at 6 * M * hidden / 8"""
    return t * (c.M * c.hidden // 8)


# ---------------------------------------------------------------------------------------------------- the layer
def _rms(x, w):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) * w


def _rope_tables(pos, dt):
    inv = 1.0 / (THETA ** (torch.arange(0, HEAD_DIM, 2, dtype=F64) / HEAD_DIM))
    ang = pos.reshape(-1)[:, None].double() * inv
    if dt == F32:                 # the device table is fp32 (vlr_rope_table)
        ang = ang.float()
    emb = torch.cat([ang, ang], -1)
    return emb.cos().to(dt), emb.sin().to(dt)


def _rope(x, cos, sin, heads, transpose=False):
    """x [M][heads * hd], rotate-half; transpose: the adjoint rotation (the backward)"""
    M = x.shape[0]
    x = x.view(M, heads, HEAD_DIM)
    x1, x2 = x[..., :HEAD_DIM // 2], x[..., HEAD_DIM // 2:]
    s = -sin if transpose else sin
    return (x * cos[:, None] + torch.cat([-x2, x1], -1) * s[:, None]).reshape(M, heads * HEAD_DIM)


def _attention(q, k, v, c, key_mask):
    B, S, nh, nkv = c.B, c.S, c.heads, c.kv_heads
    q = q.view(B, S, nh, HEAD_DIM).transpose(1, 2)
    k, v = (t.view(B, S, nkv, HEAD_DIM).transpose(1, 2).repeat_interleave(nh // nkv, dim=1) for t in (k, v))
    vis = torch.ones(S, S, dtype=torch.bool).tril()[None] & (key_mask[:, None, :] != 0)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(HEAD_DIM)
    p = torch.softmax(s.masked_fill(~vis[:, None], float("-inf")), -1)
    return (p @ v).transpose(1, 2).reshape(B * S, nh * HEAD_DIM)


def _group_shape(c, grp):
    """-> (n sub-targets, in, [out_t])"""
    H, I = c.hidden, c.inter
    Nq, Nkv = c.heads * HEAD_DIM, c.kv_heads * HEAD_DIM
    if grp == "qkv":
        return (1, H, [Nq + 2 * Nkv]) if c.nq == 1 else (3, H, [Nq, Nkv, Nkv])
    return dict(o=(1, H, [H]), gu=(2, H, [I, I]), down=(1, I, [H]))[grp]


def _adapter_term(c, sets, grp, x, rnd, fault, u_out):
    """sum over the adapter sets of u_t B_t^T for the group, [M][sum out]; the u blocks (as stored) go to u_out[(set, grp)] = [u_t]"""
    n, inn, outs = _group_shape(c, grp)
    M = x.shape[0]
    y = torch.zeros(M, sum(outs), dtype=x.dtype)
    for si, a in enumerate(sets):
        A, Bm, r = a["A_" + grp].to(x.dtype), a["B_" + grp].to(x.dtype), a["r"]
        us = []
        for i in range(n):
            keep = keep_mask(a, T0[grp] + i, M, inn, fault)
            alpha = a["scale"] / (1.0 - a["p"]) if a["p"] > 0 and fault != "no_keep_scale_u" else a["scale"]
            xd = x if keep is None else x * keep.to(x.dtype)
            u = rnd(alpha * (xd @ A[i * r:(i + 1) * r].t()))
            if a["rows"] is not None:
                u = u * a["rows"].to(x.dtype)[:, None]             # the adapter exists on the marked rows only
            us.append(u)
        if fault == "swap_gate_up_u" and grp == "gu":
            us = us[::-1]
        u_out[(si, grp)] = us
        o0 = 0
        for i in range(n):
            ui = us[i]
            if fault == "tile_skipped_with_marked_last_row" and a["rows"] is not None and _skip_on(c):
                ui = ui * _tile_live_without_last_row(a["rows"]).to(x.dtype)[:, None]
            y[:, o0:o0 + outs[i]] = y[:, o0:o0 + outs[i]] + ui @ Bm[o0:o0 + outs[i]].t()
            o0 += outs[i]
    return y


def _skip_on(c):
    return "tile_skip:on" in branches(c)


def _tile_live_without_last_row(rows):
    """bool [M]: the 256-row tiles that hold a marked row OTHER than their last one (the planted flag kernel misses that row)"""
    M = rows.numel()
    live = torch.zeros(M, dtype=torch.bool)
    for t0 in range(0, M, 256):
        t1 = min(M, t0 + 256)
        live[t0:t1] = bool(rows[t0:t1 - 1].any())
    return live


def forward(c, inp, dt, rnd, fault=None, P=None):
    """one layer; P: the parameters as a dict of tensors of dtype dt (leaves of the reference's autograd), default from inp.
    -> dict of every tensor the drivers keep"""
    P = P or params(c, inp, dt)
    sets, H, I = P["sets"], c.hidden, c.inter
    Nq, Nkv = c.heads * HEAD_DIM, c.kv_heads * HEAD_DIM
    res = (lambda t: t) if c.resid_f32 else rnd                    # the residual stream: fp32, or bf16
    cos, sin = _rope_tables(inp["pos"], dt)
    k = dict(u={})
    x_in = P["x_in"]
    k["xn1"] = rnd(_rms(x_in, P["ln1"]))
    y = k["xn1"] @ P["wqkv"].t() + _adapter_term(c, sets, "qkv", k["xn1"], rnd, fault, k["u"])
    if P["bqkv"] is not None:
        y = y + P["bqkv"]
    q, kk, v = y[:, :Nq], y[:, Nq:Nq + Nkv], y[:, Nq + Nkv:]
    k["qkv"] = rnd(torch.cat([_rope(q, cos, sin, c.heads), _rope(kk, cos, sin, c.kv_heads), v], -1))   # one rounding, after the rotation
    k["attn"] = rnd(_attention(k["qkv"][:, :Nq], k["qkv"][:, Nq:Nq + Nkv], k["qkv"][:, Nq + Nkv:], c, inp["key_mask"]))
    k["x_mid"] = res(k["attn"] @ P["wo"].t() + _adapter_term(c, sets, "o", k["attn"], rnd, fault, k["u"]) + x_in)
    k["xn2"] = rnd(_rms(k["x_mid"], P["ln2"]))
    gu = k["xn2"] @ P["wgu"].t() + _adapter_term(c, sets, "gu", k["xn2"], rnd, fault, k["u"])
    k["gu"] = rnd(gu)
    k["act"] = rnd(F.silu(gu[:, :I]) * gu[:, I:])                  # from the fp32 accumulators (csrc/gemm256p.hip, SwiGLU epilogue)
    y = k["act"] @ P["wdown"].t()
    if c.down_adapter:
        y = y + _adapter_term(c, sets, "down", k["act"], rnd, fault, k["u"])
    k["x_out"] = res(y + k["x_mid"])
    return k


def params(c, inp, dt):
    P = {n: (None if inp[n] is None else inp[n].to(dt)) for n in ("ln1", "ln2", "wqkv", "wo", "wgu", "wdown", "bqkv", "x_in")}
    P["sets"] = [{n: (v.to(dt) if isinstance(v, torch.Tensor) and v.dtype == F64 else v) for n, v in a.items()} for a in inp["sets"]]
    return P


def u_matrix(c, u):
    """the u buffer of the drivers, [M][7 r] (lora2: [M][7 (r_l + r_p)], per sub-target [u_lora | u_plora]); NaN where nothing is assigned"""
    rs = [c.r] + ([c.r_p] if c.family == "lora2" else [])
    R = sum(rs)
    some = next(iter(u.values()))[0]
    out = torch.full((some.shape[0], 7 * R), float("nan"), dtype=some.dtype)
    for (si, grp), us in u.items():
        for i, ut in enumerate(us):
            c0 = (T0[grp] + i) * R + (0 if si == 0 else rs[0])
            out[:, c0:c0 + rs[si]] = ut
    return out


def reference(c, inp):
    """float64, autograd from dy: x_out, u, dx_in, the eight adapter gradients of the trainable set and (base_grads) the six base
    gradients - the NEW gradient, before any accumulation"""
    P = params(c, inp, F64)
    leaves = {}

    def leaf(d, key, name):                                       # (a copy: the operands in `inp` stay plain tensors)
        d[key] = leaves[name] = d[key].clone().requires_grad_(True)

    leaf(P, "x_in", "x_in")
    for grp in GROUPS:
        for m in "AB":
            if P["sets"][0][f"{m}_{grp}"] is not None:
                leaf(P["sets"][0], f"{m}_{grp}", f"d{m}_{grp}")
    if c.base_grads:
        for gname, w in zip(BASE_GRADS, ("ln1", "wqkv", "wo", "ln2", "wgu", "wdown")):
            leaf(P, w, gname)
    k = forward(c, inp, F64, lambda t: t, None, P)
    grads = torch.autograd.grad((k["x_out"] * inp["dy"]).sum(), list(leaves.values()))
    out = dict(x_out=k["x_out"].detach(), u=u_matrix(c, {key: [t.detach() for t in us] for key, us in k["u"].items()}))
    for name, gr in zip(leaves, grads):
        out["dx_in" if name == "x_in" else name] = gr
    return out


# ---------------------------------------------------------------------------------------------------- replay
FAULTS = ("seed_offset", "no_keep_scale_u", "no_keep_scale_dA", "no_keep_scale_dx", "mask_compact_index", "swap_gate_up_u",
          "kv_adapter_dropped", "text_rows_leak", "accumulate_ignored", "accumulate_always", "scale_twice_dB", "plora_into_dA",
          "plora_dx_missing", "down_term_overwritten", "ln_grad_without_adapter_dx", "tile_skipped_with_marked_last_row")


# seed_offset: o_proj draws seed + 2.  no_keep_scale_u / _dA / _dx: 1 / (1 - p) missing in u, in dA, in the input-gradient term.
# mask_compact_index: a row-restricted adapter indexes its keep mask over the marked rows only.  swap_gate_up_u: the u blocks of gate and
# up change places.  kv_adapter_dropped: of the per-target launches for unequal q | k | v widths only q's runs.  text_rows_leak: v of
# o_proj is not zeroed on the text rows.  accumulate_ignored / accumulate_always: dA of gate | up overwrites / adds whatever `accumulate`
# says.  scale_twice_dB: lora_alpha / r again on dB (u is stored scaled).  plora_into_dA (lora2): the column offset into a sub-target's
# [v_lora | v_plora] block is 0 for both sides, so LoRA's columns reach the PLoRA input-gradient term.  plora_dx_missing (lora2): no
# input gradient through PLoRA.  down_term_overwritten: dx_fresh after the dgrad - d act keeps the adapter term alone.
# ln_grad_without_adapter_dx: d ln2 from dxn before the gate | up adapter term.  tile_skipped_with_marked_last_row: a 256-row tile whose
# only marked row is its last one is flagged empty and loses the row-restricted adapter's segment.


def exercises(c, fault):
    """does the case take the code the fault sits in"""
    p_any = c.dropout > 0 or (c.family == "lora2" and c.dropout_p > 0)
    rm = c.rowmask not in ("none", "zero")
    live = not (c.family == "lora_ex" and c.rowmask == "zero")       # (PLoRA alone without an image row: no adapter term anywhere)
    return {
        "seed_offset": p_any,
        "no_keep_scale_u": p_any, "no_keep_scale_dA": c.dropout > 0, "no_keep_scale_dx": p_any,
        "mask_compact_index": rm and (c.dropout_p > 0 if c.family == "lora2" else c.dropout > 0),
        "swap_gate_up_u": live,
        "kv_adapter_dropped": c.nq == 3 and c.kv_heads != c.heads,
        "text_rows_leak": rm,
        "accumulate_ignored": c.accumulate == 1, "accumulate_always": c.accumulate == 0,
        "scale_twice_dB": live,
        "plora_into_dA": c.family == "lora2" and rm, "plora_dx_missing": c.family == "lora2" and rm,
        "down_term_overwritten": c.down_adapter and live,
        "ln_grad_without_adapter_dx": c.base_grads,
        "tile_skipped_with_marked_last_row": c.rowmask == "edge" and _skip_on(c),
    }[fault]


def _vjp(fn, inputs, gout):
    ins = [t.detach().requires_grad_(True) for t in inputs]
    return torch.autograd.grad(fn(*ins), ins, gout)


def _acc(c, inp, name, new, fault, rnd):
    """the gradient buffer after the call: old + new under accumulate, one rounding"""
    acc = c.accumulate
    if name == "dA_gu" and fault == "accumulate_ignored":
        acc = 0
    if name == "dA_gu" and fault == "accumulate_always":
        acc = 1
    return rnd(new + inp["old"][name].to(new.dtype)) if acc else rnd(new)


def _group_bwd(c, inp, P, grp, x, dy, u, dx, out, rnd, fault, fresh=False):
    """lora_group_bwd / lora2_group_bwd of csrc/layers.cpp: the adapter gradients of the trainable set into `out`, the adapter terms
    of the input gradient onto dx (fresh: dx is written, not added to) -> dx"""
    n, inn, outs = _group_shape(c, grp)
    M, dt = x.shape[0], x.dtype
    two = c.family == "lora2"
    same = all(o == outs[0] for o in outs)
    term = None
    for si, a in enumerate(P["sets"]):
        A, Bm, r = a["A_" + grp], a["B_" + grp], a["r"]
        alpha = a["scale"] / (1.0 - a["p"]) if a["p"] > 0 else a["scale"]
        dAs, dBs, o0 = [], [], 0
        for i in range(n):
            dyt = dy[:, o0:o0 + outs[i]]
            dropped = fault == "kv_adapter_dropped" and not same and i > 0
            v = rnd(dyt @ Bm[o0:o0 + outs[i]])
            if a["rows"] is not None and not (fault == "text_rows_leak" and grp == "o"):
                v = v * a["rows"].to(dt)[:, None]                  # no gradient flows through the adapter on the text rows
            if dropped:
                v = torch.zeros_like(v)
            keep = keep_mask(a, T0[grp] + i, M, inn, fault)
            xd = x if keep is None else x * keep.to(dt)
            if a["train"]:
                ui = u[(si, grp)][i]
                dB = dyt.t() @ ui                                  # u is stored scaled
                if fault == "scale_twice_dB":
                    dB = dB * a["scale"]
                dBs.append(torch.zeros_like(dB) if dropped else dB)
                al = a["scale"] if fault == "no_keep_scale_dA" else alpha
                dAs.append(al * (v.t() @ xd))
            if two and si == 1 and fault == "plora_dx_missing":
                o0 += outs[i]
                continue
            vt = v
            if two and si == 1 and fault == "plora_into_dA":
                # column offset 0 for both sides: the PLoRA side reads the first r_p columns of the sub-target's [v_lora | v_plora] block
                vl = rnd(dyt @ P["sets"][0]["B_" + grp][o0:o0 + outs[i]])
                vt = torch.cat([vl, v], -1)[:, :r]
            al = a["scale"] if fault == "no_keep_scale_dx" else alpha
            t = al * (vt @ A[i * r:(i + 1) * r])
            if keep is not None:
                t = t * keep.to(dt)
            if two:                                               # lora2_group_bwd: one read-modify-write of dx per side and sub-target
                dx = rnd(t) if fresh and dx is None else rnd(dx + t)
            else:
                term = t if term is None else term + t
            o0 += outs[i]
        if a["train"]:
            out[f"dA_{grp}"] = _acc(c, inp, f"dA_{grp}", torch.cat(dAs, 0), fault, rnd)
            out[f"dB_{grp}"] = _acc(c, inp, f"dB_{grp}", torch.cat(dBs, 0), fault, rnd)
    if not two:                                                   # lora_group_bwd: ONE pass over dx for the n targets
        dx = rnd(term) if fresh and dx is None else rnd(dx + term)
    return dx


def replay(c, inp, fault=None):
    """the drivers in fp32 torch with a bf16 rounding at every bf16 store; -> the tensors reference() returns, the gradient buffers as
    they stand after the call (old + new under accumulate)"""
    assert fault is None or fault in FAULTS
    dt, rnd = F32, _bf
    P = params(c, inp, dt)
    k = forward(c, inp, dt, rnd, fault, P)
    H, I = c.hidden, c.inter
    Nq, Nkv = c.heads * HEAD_DIM, c.kv_heads * HEAD_DIM
    u, dy = k["u"], inp["dy"].to(dt)
    out = dict(x_out=k["x_out"], u=u_matrix(c, u))
    base = (lambda name, new: out.__setitem__(name, _acc(c, inp, name, new, fault, rnd))) if c.base_grads else (lambda name, new: None)
    cos, sin = _rope_tables(inp["pos"], dt)
    # ---- MLP: the adapter term of down_proj first (dx_fresh), then the dgrad with that term as its addend and the SwiGLU backward
    add = None
    if c.down_adapter:
        add = _group_bwd(c, inp, P, "down", k["act"], dy, u, None, out, rnd, fault, fresh=True)
    dg = dy @ P["wdown"]
    if add is not None and fault == "down_term_overwritten":      # dx_fresh after the dgrad: the adapter term alone is left in d act
        dact = add
    else:
        dact = rnd(dg if add is None else dg + add)
    gate, up = k["gu"][:, :I], k["gu"][:, I:]
    dgu = rnd(torch.cat(_vjp(lambda g_, u_: F.silu(g_) * u_, [gate, up], dact), -1))
    base("g_wgu", dgu.t() @ k["xn2"])
    base("g_wdown", dy.t() @ k["act"])
    dxn = rnd(dgu @ P["wgu"])
    dxn_before = dxn
    dxn = _group_bwd(c, inp, P, "gu", k["xn2"], dgu, u, dxn, out, rnd, fault)
    gx, gw = _vjp(_rms, [k["x_mid"], P["ln2"]], dxn)
    if fault == "ln_grad_without_adapter_dx":
        gw = _vjp(_rms, [k["x_mid"], P["ln2"]], dxn_before)[1]
    dx_mid = rnd(gx + dy)
    base("g_ln2", gw)
    # ---- attention
    base("g_wo", dx_mid.t() @ k["attn"])
    dattn = rnd(dx_mid @ P["wo"])
    dattn = _group_bwd(c, inp, P, "o", k["attn"], dx_mid, u, dattn, out, rnd, fault)
    qkv = k["qkv"]
    dq, dk, dv = _vjp(lambda q_, k_, v_: _attention(q_, k_, v_, c, inp["key_mask"]), [qkv[:, :Nq], qkv[:, Nq:Nq + Nkv], qkv[:, Nq + Nkv:]], dattn)
    dq, dk, dv = rnd(dq), rnd(dk), rnd(dv)
    dqkv = rnd(torch.cat([_rope(dq, cos, sin, c.heads, True), _rope(dk, cos, sin, c.kv_heads, True), dv], -1))   # vlr_rope_heads, in place
    base("g_wqkv", dqkv.t() @ k["xn1"])
    dxn = rnd(dqkv @ P["wqkv"])
    dxn = _group_bwd(c, inp, P, "qkv", k["xn1"], dqkv, u, dxn, out, rnd, fault)
    gx, gw = _vjp(_rms, [P["x_in"], P["ln1"]], dxn)
    out["dx_in"] = rnd(gx + dx_mid)
    base("g_ln1", gw)
    return out


# ---------------------------------------------------------------------------------------------------- checks
def tensors(c):
    """the compared tensors of the case"""
    names = ["x_out", "u", "dx_in"] + [n for n in LORA_GRADS if c.down_adapter or not n.endswith("_down")]
    return names + (list(BASE_GRADS) if c.base_grads else [])


def expected(c, inp, ref, name):
    """what the buffer holds after the call: old + new for a gradient under accumulate"""
    if c.accumulate and (name in LORA_GRADS or name in BASE_GRADS):
        return ref[name] + inp["old"][name]
    return ref[name]


def _select(c, inp, name, t, ref):
    """the elements of tensor `name` that are compared: x_out and the u blocks behind q|k|v on the valid rows (a padded query row is
    nobody's input), the assigned columns of u"""
    if name == "x_out":
        return t[inp["valid"]], ref[inp["valid"]]
    if name == "u":
        R = c.r + (c.r_p if c.family == "lora2" else 0)
        sel = ~torch.isnan(ref)
        sel[:, 3 * R:] &= inp["valid"][:, None]
        return t[sel], ref[sel]
    return t, ref


def err_c(c, inp, name, t, ref):
    """-> (err, scale c) of tensor `name` against the float64 reference; a gradient under accumulate is compared after the known old
    value is taken off, so that c keeps measuring the NEW gradient's scale"""
    t, ref = t.double(), ref.double()
    if c.accumulate and (name in LORA_GRADS or name in BASE_GRADS):
        t = t - inp["old"][name]
    t, ref = _select(c, inp, name, t, ref)
    top = float(ref.abs().max())
    if not bool(torch.isfinite(t).all()):
        return float("inf"), float("nan")
    if top == 0.0:                                                # the reference is exactly zero: so must the tensor be
        return (0.0 if float(t.abs().max()) == 0.0 else float("inf")), 1.0
    return float((t - ref).abs().max()) / top, float((t * ref).sum() / (ref * ref).sum())


def bounds(err_replay, c_replay):
    return MARGIN * err_replay, MARGIN * abs(c_replay - 1.0) + C_FLOOR


def measure(c, inp, ref, got):
    """{tensor: (err, c)}"""
    return {n: err_c(c, inp, n, got[n], ref[n]) for n in tensors(c)}


def ratios(meas, meas_replay):
    """{tensor: (err / bound, |c - 1| / bound)}; a tensor whose bound is 0 must have err 0 (ratio 0), else inf"""
    out = {}
    for n, (e, cc) in meas.items():
        be, bc = bounds(*meas_replay[n])
        re_ = 0.0 if e == 0.0 else (float("inf") if be == 0.0 else e / be)
        rc = float("inf") if cc != cc else abs(cc - 1.0) / bc
        out[n] = (re_, rc)
    return out
