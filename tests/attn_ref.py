"""Reference attention for the kernel tests (plain module, no pytest hooks).

Layout everywhere: q [B, S, heads, D], k / v [B, S, kv_heads, D], key_mask [B, S] (0 = masked key) or None, dO like q.  Query head h
reads K/V head h // group.  lse is returned token-major, [B, S, heads], in the log2 domain the kernels store (log2 sum_j 2^(s_j scale
log2 e)); a query that sees no key has O = 0 and lse = +inf.

  ref_attention            fp64, one (sequence, head) at a time, on the inputs' device
  emulate_kernel_rounding  the same attention with the kernels' roundings (bf16 operands, fp32 scores and online softmax over 64-key
                           tiles, P and dS rounded to bf16 before their products, bf16 outputs); `bug=` injects one of BUGS
  check_tiles              per (sequence, head, 64-row tile) error against the reference, exact where the reference is structurally 0
"""
import math
from collections import namedtuple

import torch

LOG2E = 1.0 / math.log(2.0)
KV_TILE = 64
# a tile's error is divided by max(largest |ref| in the tile, FLOOR * largest |ref| of its (sequence, head), ABS_FLOOR): tiles of
# near-zero gradient would otherwise turn fp32 / bf16 noise into large relative errors.  The inputs are O(1); ABS_FLOOR only matters
# where the exact gradient of a whole head vanishes (dQ and dK when every row sees one key, S = 1)
FLOOR = 1.0 / 16
ABS_FLOOR = 1e-3

# o, dq [B, S, heads, D]; lse [B, S, heads]; dk, dv [B, S, kv_heads, D] (None without dO).  Structural zeros, exact in every
# implementation: zero_q [B, S, heads] = query rows that see no key (O = 0, lse = +inf, dQ = 0); zero_dq adds the rows whose dO is 0;
# zero_kv [B, S, kv_heads] = keys that no query with a nonzero dO sees (dK = dV = 0).
Attn = namedtuple("Attn", "o lse dq dk dv zero_q zero_dq zero_kv")

BUGS = ("diag_dropped",          # causal compare key >= q instead of key > q: the diagonal key is masked
        "future_key",            # causal compare key > q + 1: one future key is admitted
        "tail_tile_ignored",     # the keys of the last, partial KV tile are skipped
        "no_rescale",            # the accumulator is not rescaled when the running maximum moves (l is)
        "gqa_mod",               # query head h reads K/V head h % kv_heads instead of h // group
        "mask_tile_ignored",     # the key mask is not applied on the first KV tile that holds a masked key
        "dk_scale_tile",         # dK of one 64-key tile (the last one with a nonzero dK) is written without the softmax scale
        "noncausal_as_causal")   # a non-causal call computes causal attention


def visibility(S, km_row, causal, device, bug=None):
    """[S, S] bool: query i sees key j"""
    vis = torch.ones(S, S, dtype=torch.bool, device=device)
    if causal:
        vis = vis.tril({"diag_dropped": -1, "future_key": 1}.get(bug, 0))
    elif bug == "noncausal_as_causal":
        vis = vis.tril()
    if km_row is not None:
        ok = km_row != 0
        if bug == "mask_tile_ignored" and bool((~ok).any()):
            j = int((~ok).nonzero()[0]) // KV_TILE * KV_TILE
            ok = ok.clone()
            ok[j:j + KV_TILE] = True
        vis = vis & ok[None, :]
    if bug == "tail_tile_ignored" and S % KV_TILE:
        vis[:, S // KV_TILE * KV_TILE:] = False
    return vis


def _structure(vis_list, do, B, S, nh, nkv, group, device):
    zero_q = torch.zeros(B, S, nh, dtype=torch.bool, device=device)
    zero_kv = torch.ones(B, S, nkv, dtype=torch.bool, device=device)
    for b in range(B):
        vis = vis_list[b]
        zero_q[b] = (~vis.any(1))[:, None]
        if do is not None:
            live = do[b].ne(0).any(-1)                                        # [S, nh]: rows with a nonzero dO
            for h in range(nh):
                zero_kv[b, :, h // group] &= ~(vis & live[:, h, None]).any(0)
    zero_dq = zero_q | ~do.ne(0).any(-1) if do is not None else zero_q
    return zero_q, zero_dq, zero_kv


def ref_attention(q, k, v, key_mask=None, causal=True, scale=None, group=None, do=None, o_bwd=None):
    """fp64 attention (and, for dO = `do`, its gradients), one (sequence, head) at a time; K/V-head gradients summed over the group.
    o_bwd [B, S, heads, D]: the O the backward is given.  The kernels' backward takes the forward's bf16 O as an input and forms
    delta = rowsum(dO * O) from it; where one key dominates a row, dP - delta cancels to the rounding of O, so the exact gradient of
    that backward is the one with delta from o_bwd (None: from the exact O)."""
    B, S, nh, D = q.shape
    nkv = k.shape[2]
    group = group or nh // nkv
    assert nh == nkv * group
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    dev, f = q.device, torch.float64
    o = torch.zeros(B, S, nh, D, dtype=f, device=dev)
    lse = torch.full((B, S, nh), math.inf, dtype=f, device=dev)
    dq = torch.zeros_like(o) if do is not None else None
    dk = torch.zeros(B, S, nkv, D, dtype=f, device=dev) if do is not None else None
    dv = torch.zeros_like(dk) if do is not None else None
    vis_list = []
    for b in range(B):
        vis = visibility(S, None if key_mask is None else key_mask[b], causal, dev)
        vis_list.append(vis)
        seen = vis.any(1)
        for h in range(nh):
            kvh = h // group
            qh, kh, vh = q[b, :, h].to(f), k[b, :, kvh].to(f), v[b, :, kvh].to(f)
            s = ((qh @ kh.t()) * scale).masked_fill(~vis, -math.inf)
            ln = torch.logsumexp(s, 1).masked_fill(~seen, 0.0)
            p = torch.exp(s - ln[:, None])                                   # masked scores: exactly 0
            oh = p @ vh
            o[b, :, h] = oh
            lse[b, :, h] = torch.where(seen, ln * LOG2E, torch.full_like(ln, math.inf))
            if do is not None:
                doh = do[b, :, h].to(f)
                dp = doh @ vh.t()
                delta = (doh * (oh if o_bwd is None else o_bwd[b, :, h].to(dev, f))).sum(1)
                ds = p * (dp - delta[:, None])
                dq[b, :, h] = (ds @ kh) * scale
                dk[b, :, kvh] += (ds.t() @ qh) * scale
                dv[b, :, kvh] += p.t() @ doh
            del s, p
    zero_q, zero_dq, zero_kv = _structure(vis_list, do, B, S, nh, nkv, group, dev)
    return Attn(o, lse, dq, dk, dv, zero_q, zero_dq, zero_kv)


def _bf16(x):
    return x.to(torch.bfloat16).float()


def emulate_kernel_rounding(q, k, v, key_mask=None, causal=True, scale=None, group=None, do=None, bug=None):
    """The kernels' arithmetic in fp32 on bf16 operands: scores fp32, online softmax over 64-key tiles in the log2 domain (running max
    m, sum l, accumulator rescaled by 2^(m_old - m_new)), P rounded to bf16 before P.V, O rounded to bf16; backward: P = 2^(s sl2 - lse),
    delta = rowsum(dO * O_bf16), dS = P (dP - delta) rounded to bf16 before dS.K and dS^T.Q, P rounded to bf16 before P^T.dO, fp32
    accumulation over the group, bf16 outputs.  `bug` (one of BUGS) turns it into a model of a wrong kernel."""
    assert bug is None or bug in BUGS, bug
    B, S, nh, D = q.shape
    nkv = k.shape[2]
    group = group or nh // nkv
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    sl2 = scale * LOG2E
    dev, f = q.device, torch.float32
    o = torch.zeros(B, S, nh, D, dtype=f, device=dev)
    lse = torch.full((B, S, nh), math.inf, dtype=f, device=dev)
    dq = torch.zeros_like(o) if do is not None else None
    dk = torch.zeros(B, S, nkv, D, dtype=f, device=dev) if do is not None else None
    dv = torch.zeros_like(dk) if do is not None else None
    vis_list = []
    for b in range(B):
        vis = visibility(S, None if key_mask is None else key_mask[b], causal, dev, bug)
        vis_list.append(vis)
        for h in range(nh):
            kvh = h % nkv if bug == "gqa_mod" else h // group
            qh, kh, vh = _bf16(q[b, :, h]), _bf16(k[b, :, kvh]), _bf16(v[b, :, kvh])
            s = (qh @ kh.t()).masked_fill(~vis, -math.inf)
            m = torch.full((S,), -math.inf, dtype=f, device=dev)
            l = torch.zeros(S, dtype=f, device=dev)
            acc = torch.zeros(S, D, dtype=f, device=dev)
            for k0 in range(0, S, KV_TILE):
                st = s[:, k0:k0 + KV_TILE]
                m_new = torch.maximum(m, st.max(1).values * sl2)
                m_use = m_new.masked_fill(m_new == -math.inf, 0.0)
                alpha = torch.exp2(m - m_use)
                p = torch.exp2(st * sl2 - m_use[:, None])
                l = l * alpha + p.sum(1)
                if bug != "no_rescale":
                    acc = acc * alpha[:, None]
                acc = acc + _bf16(p) @ vh[k0:k0 + KV_TILE]
                m = m_new
            inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
            oh = _bf16(acc * inv[:, None])
            o[b, :, h] = oh
            lh = torch.where(l > 0, m + torch.log2(l), torch.full_like(l, math.inf))
            lse[b, :, h] = lh
            if do is not None:
                doh = _bf16(do[b, :, h])
                p = torch.exp2(s * sl2 - lh[:, None])                      # masked scores and lse = +inf: exactly 0
                dp = doh @ vh.t()
                delta = (doh * oh).sum(1)
                ds = _bf16(p * (dp - delta[:, None]))
                dq[b, :, h] = _bf16((ds @ kh) * scale)
                dk[b, :, kvh] += (ds.t() @ qh) * scale
                dv[b, :, kvh] += _bf16(p).t() @ doh
    zero_q, zero_dq, zero_kv = _structure(vis_list, do, B, S, nh, nkv, group, dev)
    if do is not None:
        dk, dv = _bf16(dk), _bf16(dv)
        if bug == "dk_scale_tile":
            live = (~zero_kv).any(0).any(-1).nonzero()
            if len(live):
                j = int(live[-1]) // KV_TILE * KV_TILE
                dk[:, j:j + KV_TILE] = _bf16(dk[:, j:j + KV_TILE] / scale)
    return Attn(o, lse, dq, dk, dv, zero_q, zero_dq, zero_kv)


def tile_errors(out, ref, rows=KV_TILE):
    """[B, H, ntiles] errors of out against ref, both [B, S, H, ...]: largest |out - ref| in the tile / max(largest |ref| in the tile,
    FLOOR * largest |ref| of the (sequence, head)).  Where ref is +inf, out must equal it; a non-finite out elsewhere is an infinite
    error."""
    B, S, H = ref.shape[:3]
    r = ref.to(torch.float64).reshape(B, S, H, -1)
    x = out.to(r.device).to(torch.float64).reshape(B, S, H, -1)
    inf = torch.isinf(r)
    err = (x - r).abs()
    err = torch.where(inf, torch.where(x == r, 0.0, math.inf), err)
    err = torch.where(torch.isnan(err) | (torch.isinf(x) & ~inf), math.inf, err)
    mag = r.abs().masked_fill(inf, 0.0)
    nt = (S + rows - 1) // rows
    pad = nt * rows - S
    if pad:
        err = torch.nn.functional.pad(err, (0, 0, 0, 0, 0, pad))
        mag = torch.nn.functional.pad(mag, (0, 0, 0, 0, 0, pad))
    err = err.reshape(B, nt, rows, H, -1).amax(dim=(2, 4))                  # [B, nt, H]
    mag = mag.reshape(B, nt, rows, H, -1).amax(dim=(2, 4))
    den = torch.maximum(mag, FLOOR * mag.amax(1, keepdim=True)).clamp_min(ABS_FLOOR)
    return (err / den).permute(0, 2, 1)                                      # [B, H, nt]


def check_tiles(out, ref, tol, rows=KV_TILE, zero=None, what=""):
    """Asserts that every (sequence, head, `rows`-row tile) of out [B, S, H, ...] is within tol of ref (tile_errors), and that the rows
    of the bool mask `zero` [B, S, H] are exactly what ref holds there: 0, or +inf for the lse of a row that sees no key.  Returns the
    worst tile error."""
    if zero is not None and bool(zero.any()):
        z = zero.to(ref.device)
        rz, xz = ref[z].to(torch.float64), out.to(ref.device)[z].to(torch.float64)
        assert bool(((rz == 0) | (rz == math.inf)).all()), f"{what}: reference not 0 / +inf on its structural zero rows"
        bad = (xz != rz).reshape(rz.shape[0], -1).any(1)
        if bool(bad.any()):
            b, s, h = z.nonzero()[bad.nonzero()[0, 0]].tolist()
            raise AssertionError(f"{what}: (b, s, h) = ({b}, {s}, {h}) must be exactly {'+inf' if bool(torch.isinf(rz).any()) else 0}, "
                                 f"{int(bad.sum())} such rows differ")
    e = tile_errors(out, ref, rows)
    worst = float(e.max())
    if not worst <= tol:
        b, h, t = [int(i) for i in torch.nonzero(e == e.max())[0]]
        raise AssertionError(f"{what}: tile error {worst:.3e} > {tol:.1e} at (b, h, tile) = ({b}, {h}, {t}), rows {t * rows}..")
    return worst


# ---------------------------------------------------------------------------------------------------- the case matrix
# kind: "resampler" (non-causal, the first nq keys masked, dO only on those nq rows: engine_qwen.resampler_*), "right" / "holes" /
# "left" (key masks: right padding, interior holes, left padding of pads[b] keys in sequence b), "none".  scores: "normal" (N(0, 1)
# q, k: unit score variance), "sink" (the first valid key of every sequence scores ~40 above the rest), "spike" (a key in each row's
# last KV tile scores ~40 above the rest: the diagonal when causal, the last valid key when not), "rising" (the row maximum rises by
# 40 / (tiles - 1) per KV tile), "std8" (score std ~8).
Case = namedtuple("Case", "group name B S nh nkv D causal kind scores nq pads bwd")


def _case(group, B, S, nh=2, nkv=None, D=128, causal=True, kind="none", scores="normal", nq=0, pads=(), bwd=True, name=None):
    nkv = nkv or nh
    name = name or (f"{group}-B{B}-S{S}-h{nh}/{nkv}-d{D}-{'c' if causal else 'nc'}-{kind}-{scores}" + (f"-nq{nq}" if nq else "")
                    + ("" if bwd else "-fwd"))
    return Case(group, name, B, S, nh, nkv, D, causal, kind, scores, nq, tuple(pads), bwd)


def cases(max_S=None):
    """the parity matrix of tests/test_hip_attention_edges.py; max_S keeps the cases with S <= max_S"""
    out = []
    for nq in (16, 64, 256):
        for T in (64, 200):
            out.append(_case("resampler", 2, nq + T, causal=False, kind="resampler", nq=nq))
    out.append(_case("resampler", 2, 256 + 1024, nh=32, causal=False, kind="resampler", nq=256, name="resampler-real-n2-nq256-T1024-h32"))
    for kind in ("right", "holes"):
        out.append(_case("resampler", 2, 200, causal=False, kind=kind))
    for S in (200, 700):
        for causal in (True, False):
            out.append(_case("masks", 5, S, causal=causal, kind="left", pads=(0, 7, 64, 130, 300)))
    for S in (1, 2, 31, 33, 63, 64, 65, 127, 128, 129, 255, 257):
        for causal in (True, False):
            out.append(_case("lengths", 2, S, causal=causal, kind="right" if S > 8 else "none"))
        out.append(_case("lengths", 2, S, D=64, causal=False, bwd=False))
    for nh, nkv in ((8, 8), (8, 4), (8, 2), (8, 1), (16, 2), (12, 4)):
        out.append(_case("groups", 2, 200, nh=nh, nkv=nkv, kind="left", pads=(0, 70)))
        out.append(_case("groups", 2, 200, nh=nh, nkv=nkv, causal=False, kind="right"))
    for S in (129, 1599):
        for scores in ("sink", "spike", "rising", "std8"):
            out.append(_case("scores", 1, S, scores=scores, kind="right"))
            if S == 129:
                out.append(_case("scores", 1, S, causal=False, scores=scores, kind="right"))
    out.append(_case("long", 1, 8200, kind="right"))     # past ATTN_MAX_TILES * KV_TILE = 8192: the register-staged kernels
    return [c for c in out if max_S is None or c.S <= max_S]


# Per-tile tolerances of each case group: about 2x the worst tile error of emulate_kernel_rounding against ref_attention over the
# group's cases (tests/test_attn_checker_host.py checks the model passes them).  Worst emulation errors, o / lse / dq / dk / dv:
#   resampler 4.3e-3 / 1.0e-7 / 5.8e-3 / 6.2e-3 / 6.4e-3     masks  3.9e-3 / 1.1e-7 / 5.9e-3 / 5.3e-3 / 5.6e-3
#   lengths   4.5e-3 / 1.1e-7 / 6.6e-3 / 5.5e-3 / 4.4e-3     groups 4.7e-3 / 1.2e-7 / 6.3e-3 / 5.3e-3 / 5.3e-3
#   scores    3.7e-3 / 3.4e-7 / 3.7e-2 / 5.5e-3 / 4.6e-3     long   3.5e-3 / 1.1e-7 / 4.6e-3 / 4.9e-3 / 4.2e-3
# dQ of the score-range cases: the keys carry a large common component (sink, rising maximum) and dQ = sum_j dS_ij k_j with dS
# rounded to bf16 no longer has its exact zero row sum, so the rounding of dS is multiplied by |k|
TOL = dict(resampler=dict(o=8.6e-3, lse=2.1e-7, dq=1.2e-2, dk=1.3e-2, dv=1.3e-2),
           masks=dict(o=7.8e-3, lse=2.1e-7, dq=1.2e-2, dk=1.1e-2, dv=1.2e-2),
           lengths=dict(o=9.0e-3, lse=2.3e-7, dq=1.3e-2, dk=1.1e-2, dv=8.8e-3),
           groups=dict(o=9.4e-3, lse=2.4e-7, dq=1.3e-2, dk=1.1e-2, dv=1.1e-2),
           scores=dict(o=7.4e-3, lse=6.8e-7, dq=7.5e-2, dk=1.1e-2, dv=9.3e-3),
           long=dict(o=7.0e-3, lse=2.1e-7, dq=9.3e-3, dk=9.8e-3, dv=8.4e-3))


def key_mask_of(c):
    """[B, S] int32 key mask of case c (None for kind 'none')"""
    B, S = c.B, c.S
    if c.kind == "none":
        return None
    km = torch.ones(B, S, dtype=torch.int32)
    if c.kind == "resampler":
        km[:, :c.nq] = 0
    elif c.kind == "right":
        km[0, S - max(1, S // 9):] = 0
    elif c.kind == "holes":
        for b in range(B):
            km[b, 40 + 3 * b:40 + 3 * b + 70] = 0              # covers the whole KV tile 64..127
            km[b, 150 + b::17] = 0
    elif c.kind == "left":
        for b in range(B):
            km[b, :min(S, c.pads[b % len(c.pads)])] = 0
    return km


def make_inputs(c, seed=0):
    """bf16 q [B, S, nh, D], k, v [B, S, nkv, D], dO [B, S, nh, D] (None without a backward) and the key mask of case c, on the CPU"""
    g = torch.Generator().manual_seed(seed)
    B, S, nh, nkv, D = c.B, c.S, c.nh, c.nkv, c.D
    q = torch.randn(B, S, nh, D, generator=g)
    k = torch.randn(B, S, nkv, D, generator=g)
    v = torch.randn(B, S, nkv, D, generator=g)
    do = torch.randn(B, S, nh, D, generator=g) if c.bwd else None
    km = key_mask_of(c)
    ok = torch.ones(B, S, dtype=torch.bool) if km is None else km != 0
    u = torch.randn(D, generator=g)
    u = u / u.norm()
    sq = math.sqrt(D)                                                     # score = (q . k) / sqrt(D)
    if c.scores in ("sink", "rising") or (c.scores == "spike" and not c.causal):
        q = q + 4.0 * u                                                   # q . u ~ 4 +- 1
    if c.scores == "sink":
        for b in range(B):
            j = ok[b].nonzero()
            if len(j):
                k[b, int(j[0])] += 10.0 * sq * u                          # score ~ +40
    elif c.scores == "spike" and c.causal:
        # k_i += 40 sqrt(D) q_i / |q_i|^2 (the group's first query head): the diagonal scores ~40 above the rest of row i
        qg = q[:, :, ::nh // nkv]
        k = k + 40.0 * sq * qg / (qg * qg).sum(-1, keepdim=True)
    elif c.scores == "spike":
        for b in range(B):
            j = ok[b].nonzero()
            if len(j):
                k[b, int(j[-1])] += 10.0 * sq * u
    elif c.scores == "rising":
        step = 40.0 / max(1, (S - 1) // KV_TILE)
        t = (torch.arange(S) // KV_TILE).float()
        k = k + (step * sq / 4.0) * t[None, :, None, None] * u
    elif c.scores == "std8":
        q = q * 8.0
    if c.kind == "resampler":
        do[:, c.nq:] = 0                                                  # only the query rows carry a gradient
    bf = lambda x: None if x is None else x.to(torch.bfloat16)           # noqa: E731
    return bf(q), bf(k), bf(v), bf(do), km


def check_attention(res, ref, tol, what="", fwd_only=False):
    """check_tiles for every output of `res` (an Attn, any float dtype) against `ref`; tol = dict(o=, lse=, dq=, dk=, dv=).
    -> {output: worst tile error}"""
    worst = dict(o=check_tiles(res.o, ref.o, tol["o"], zero=ref.zero_q, what=what + " O"),
                 lse=check_tiles(res.lse, ref.lse, tol["lse"], zero=ref.zero_q, what=what + " lse"))
    if not fwd_only and ref.dq is not None:
        worst["dq"] = check_tiles(res.dq, ref.dq, tol["dq"], zero=ref.zero_dq, what=what + " dQ")
        worst["dk"] = check_tiles(res.dk, ref.dk, tol["dk"], zero=ref.zero_kv, what=what + " dK")
        worst["dv"] = check_tiles(res.dv, ref.dv, tol["dv"], zero=ref.zero_kv, what=what + " dV")
    return worst
