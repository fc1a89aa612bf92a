"""Reference, case table and checker inputs for the fused-epilogue GEMMs of csrc/gemm256p.hip (plain module, no pytest hooks; CPU only
unless a device is named): gate | up + SwiGLU (fuse 1), q | k | v + bias + rotate-half RoPE (fuse 2), the down projection's dgrad + SwiGLU
backward (fuse 3), and the first two with a LoRA adapter segment riding the K loop.  tests/test_fused_gemm_checker_host.py runs the
checker on the CPU, tests/test_hip_fused_gemm_edges.py runs the same cases on the GPU.  Buffers, the checker and its conventions are those
of tests/row_ref.py and tests/gemm_ref.py.

  CASES                one Case per launch: op ("swiglu" | "rope" | "bwd"), the shape, the data regime, the variant (store_gu, bias and its
                       offset, rope_cols, head_dim, the addend and its alias, the adapter rank and block widths) and n256: the launches of
                       gemm256p_kernel the in-library profiler must count - 1 = the fused route, 0 = the fallback of include/vlr.h
  make(c)              CPU operands as Bufs: x with ldx = K + 8 and NaN in the padding, NaN guard cells in front of and behind every buffer,
                       GUARD_ROWS NaN rows behind row M of every [M][.] buffer (gu, act, qkv, dact_ws, dact_add, x, u, dy); outputs
                       pre-filled with NaN (gate | up of the backward: with the forward's values); the cos / sin tables behind guards
  expect(c, inp)       {output: Exp} in float64, following the route (below)
  emulate(c, inp)      {output: tensor}: the same in torch fp32, rounded where the route rounds
  outputs(c)           every buffer the call may write; the ones expect() does not name are scratch - only their guards are checked
  sample(c)            rows (every 128 / 256 tile edge, the corners, a few others) for the host test of a multi-tile case; all columns

What the routes compute (G = x Wg^T, U = x Wu^T, P = x W^T + bias, D = dy Wdown + addend; "+ u Bl^T" on the adapter entry points):
  fused     the elementwise step runs on the fp32 accumulators, every output is rounded ONCE:
            gu = bf16([G | U]), act = bf16(silu(G) U);  qkv = bf16(rot(P));  [d gate | d up] = bf16(swiglu'(gate, up) D)
  fallback  the plain GEMM rounds its result to bf16 first (gemm_swiglu_impl, gemm_qkv_rope_impl, gemm_swiglu_bwd_impl in csrc/gemm.hip):
            gu = bf16([G | U]) then vlr_swiglu_fwd on gu;  bf16(P) then vlr_rope_heads in place;  dact_ws = bf16(D) then vlr_swiglu_bwd.
            With an adapter, seg_fallback_add reads the rounded base product back, adds u Bl^T in fp32 and rounds again.
            Fallback cases exist in the exact regimes only: there the rounded intermediate is determined, and the reference is built from it.

The data regimes.
  exact     x, W (dy, Wdown) uniform integers in [-8, 8]; for the two SwiGLU ops x (dy) carries 2^-6, so that gate, up and d act spread over
            roughly [-8, 8] where silu is curved; the bias integers within +-64 times a power of two per head, the addend integers / 16.
            make() asserts sum |a||b| + |bias| + |addend| < 2^24 units per element: every fp32 partial sum in every order is exact.
            gu, and the WHOLE q | k | v + RoPE output, are then BITWISE the float64 result rounded once to bf16: the RoPE cases get PLANTED
            cos / sin tables with entries from {0, +-1/4, +-1/2, +-1, +-2} chosen by a hash of (table, position, feature) - x1 c - x2 s is
            exact in fp32, and a wrong position, feature or partner changes bits.  act and d gate | d up go through fast_sigmoid and get the
            bound below without its accumulator term.
  exact256  sparse +-1 data, asserted sum of |terms| <= 256: every intermediate is exact in bf16 too (adapter fallbacks, which round twice)
  gauss     randn * 0.5 (gate | up of the backward: randn * 2, addend randn); RoPE tables as vlr_rope_table writes them, READ BACK by the GPU
            test and treated as float inputs (on the CPU: cos / sin in float64 rounded to fp32).  ELEMENTWISE
            |out - ref64| <= 2^-8 |ref| + coef (accumulator magnitude through the epilogue's partial derivatives) + arithmetic term;
            coef = (K + r + 6) 2^-23 as in gemm_ref, accumulator magnitude mX = |x|.|W| (+ |u|.|Bl| + |bias| + |addend|) in float64:
              gu            coef mX
              act           coef (1.1 |U| mG + |silu(G)| mU) + (4 2^-24 + TOL["fwd"]) max(|act|, |silu(G)|)      |d silu / d g| <= 1.0998
              rot           y1 = x1 c - x2 s, y2 = x2 c + x1 s:  coef (|c| m1 + |s| m2) + 4 2^-24 (|x1 c| + |x2 s|), and likewise y2
              d gate, d up  linear in D: coef mD |u sg (1 + g (1 - sg))| resp. coef mD |g sg|, + (6 2^-24 + TOL["bwd"]) times row_ref's
                            magnitudes |D u sg| (1 + |g| (1 + sg)) resp. |D g sg|
            fast_sigmoid = v_rcp_f32(1 + __expf(-x)) has no derivable bound.  TOL holds the worst error of the fp32 epilogue against the
            float64 epilogue over this module's cases, on the CPU, in units of the magnitudes above, and 4x that as the allowance
            (`python -m tests.fused_gemm_ref`, measure_tol() below; both see the accumulators rounded to fp32, so only the epilogue counts).
Nothing here is derived from a kernel's output.

The peeled "fused tail" launches are unreachable (checked: peel_tail256_best() below restates choose_peel of csrc/gemm.hip).  With
tail256 = true a peel of r tile rows is accepted only if ceil(kept / ncu) + 1.15 ceil(peeled / ncu) < ceil(all / ncu) - 0.05; but
ceil(x) + ceil(y) >= ceil(x + y) and peeled >= 1, so the left side is never below the right for any M, N and CU count: choose_peel(...,
true) returns 0 always, and the second launches in gemm_swiglu_impl, gemm_qkv_rope_impl, gemm_swiglu_bwd_impl (and vlr_gemm_swiglu_bwd_src)
never run - the (12792, 2048, 256) case of test_hip_kernels.py does not cover "a peeled tail".  No case is spent on that branch.
"""
import torch

from tests.row_ref import logical, check, check_poison, worst_ratio, Exp, Buf, GUARD, U_BF16, U_F32, rope_tables_f32   # noqa: F401 (re-exported)
from tests.gemm_ref import Case, U_MFMA, DEVICE_REF_MACS, row_bits, _edges                                              # noqa: F401

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
GUARD_ROWS = 2
MAX_POS = 40
NAN = float("nan")

# (measured worst |fp32 epilogue - float64 epilogue| / magnitude over this module's cases, allowance = 4x measured).
# Obtained with `python -m tests.fused_gemm_ref` (measure_tol() below, CPU).  row_ref.TOL["swiglu_fwd"] / ["swiglu_bwd"] measured 2.1e-7 and
# 2.3e-7 on their own data: not equal, so not reused.
TOL = {"fwd": (2.0e-7, 7.9e-7), "bwd": (2.5e-7, 1.0e-6)}


# ---------------------------------------------------------------------------------------------------- the case table
def _sw(M, I, K, n256, regime="exact", store_gu=1, r=0, tag=""):
    name = f"swiglu-{M}x{I}x{K}-{regime}-gu{store_gu}" + (f"-r{r}" if r else "") + (f"-{tag}" if tag else "")
    return Case(name=name, op="swiglu", M=M, I=I, N=2 * I, K=K, ldx=K + 8, n256=n256, regime=regime, store_gu=store_gu, r=r, ldu=2 * r + 16,
                blocks=(I, 2 * I) if r else (), seed=(M * 31 + I * 17 + K * 7 + r) % 100003)


def _rp(M, K, nh, nkv, n256, regime="exact", hd=128, bias=None, rope_cols=None, r=0, qkv_cols=None, tag=""):
    """bias: None | 0 | 4 | 1 = none / elements the bias sits behind a 16-byte aligned address (4: 8-byte aligned, fused; 1: the fallback)
    qkv_cols: (q_cols, kv_cols) of vlr_gemm_qkv_rope_lora, kv_cols = 0 the single-adapter form"""
    N = (nh + 2 * nkv) * hd
    rope_cols = (nh + nkv) * hd if rope_cols is None else rope_cols
    name = f"rope-{M}x{K}x{nh}+{nkv}-{regime}-hd{hd}-rc{rope_cols}" + (f"-bias{bias}" if bias is not None else "") + (f"-r{r}" if r else "") + \
        (f"-{tag}" if tag else "")
    nb = 0 if not r else (1 if not qkv_cols[1] else 3)
    blocks = () if not r else ((N,) if nb == 1 else (qkv_cols[0], qkv_cols[0] + qkv_cols[1], N))
    return Case(name=name, op="rope", M=M, N=N, K=K, ldx=K + 8, hd=hd, rope_cols=rope_cols, bias=bias, n256=n256, regime=regime, r=r,
                ldu=nb * r + 16, blocks=blocks, qkv_cols=qkv_cols, tables="device" if regime == "gauss" else "planted",
                seed=(M * 29 + N * 13 + K * 5 + r + (bias or 0)) % 100003)


def _bw(M, I, H, n256, regime="exact", add=None, tag=""):
    """add: None | "sep" | "alias" (dact_add == dact_ws)"""
    name = f"bwd-{M}x{I}x{H}-{regime}" + (f"-add{add}" if add else "") + (f"-{tag}" if tag else "")
    return Case(name=name, op="bwd", M=M, I=I, N=I, K=H, n256=n256, regime=regime, add=add, r=0, seed=(M * 37 + I * 11 + H * 3) % 100003)


MULTI = {"swiglu": (4104, 2056, 256), "rope": (4104, 256, 30, 2), "bwd": (4104, 4104, 256)}      # 17 x 17 tiles each: workgroups walk two


def _build_cases():
    cs = []
    # ---- vlr_gemm_swiglu: one partial tile at the shallowest K; 256 + 8 rows, 128 + 8 gate columns, K % 64 = 8; one row tile, one full
    # column tile, five K tiles; three row tiles x five column tiles with 8 columns in the last; K < 256: the fallback
    for g in (1, 0):
        cs += [_sw(8, 8, 256, 1, store_gu=g), _sw(264, 136, 264, 1, store_gu=g), _sw(37, 128, 320, 1, store_gu=g),
               _sw(549, 520, 256, 1, store_gu=g), _sw(300, 136, 200, 0, store_gu=g)]
    cs += [_sw(264, 136, 264, 1, "gauss", store_gu=g) for g in (1, 0)] + [_sw(549, 520, 256, 1, "gauss")]
    cs += [_sw(*MULTI["swiglu"], 1), _sw(*MULTI["swiglu"], 1, "gauss", store_gu=0)]
    # ---- vlr_gemm_qkv_rope[_bias]: two rotated tiles + one v tile; GQA, N = 1024, rope_cols = 768; everything rotated; nothing rotated
    for b in (None, 0):
        cs += [_rp(8, 256, 2, 2, 1, bias=b), _rp(264, 264, 4, 2, 1, bias=b), _rp(37, 256, 2, 0, 1, bias=b),
               _rp(8, 256, 2, 2, 1, bias=b, rope_cols=0)]
        # fallbacks: N = 384 is no multiple of 256; head_dim 64; K < 256
        cs += [_rp(300, 256, 1, 1, 0, bias=b), _rp(37, 256, 4, 2, 0, hd=64, bias=b), _rp(37, 200, 2, 2, 0, bias=b)]
    # the bias 8 bytes behind a 16-byte boundary stays fused, 2 bytes behind one falls back
    cs += [_rp(264, 264, 4, 2, 1, bias=4), _rp(264, 264, 4, 2, 0, bias=1)]
    cs += [_rp(264, 264, 4, 2, 1, "gauss", bias=b) for b in (None, 0, 4)] + [_rp(37, 256, 2, 0, 1, "gauss", bias=0)]
    cs += [_rp(*MULTI["rope"], 1, bias=0), _rp(*MULTI["rope"], 1, "gauss", bias=0)]
    # ---- vlr_gemm_swiglu_bwd[_add]
    for M, I, H, n in ((8, 8, 256, 1), (264, 264, 264, 1), (37, 512, 256, 1), (549, 520, 256, 1), (549, 520, 128, 0)):
        cs += [_bw(M, I, H, n)]
    for M, I, H, n in ((264, 264, 264, 1), (549, 520, 256, 1), (549, 520, 128, 0)):
        cs += [_bw(M, I, H, n, add=a) for a in ("sep", "alias")]
    cs += [_bw(264, 264, 264, 1, "gauss"), _bw(549, 520, 256, 1, "gauss", add="sep"), _bw(264, 264, 264, 1, "gauss", add="alias")]
    cs += [_bw(*MULTI["bwd"], 1), _bw(*MULTI["bwd"], 1, "gauss", add="sep")]
    # ---- the adapter segment (vlr_gemm256p_seg_try_launch: K >= 256 and K % 64 == 0, N and rope_cols multiples of 256, block bounds
    # below N on 256-column tile edges; no minimum tile count): the smallest fused shapes at r = 8 and r = 128, ldu = blocks * r + 16
    for r in (8, 128):
        cs += [_sw(8, 8, 256, 1, r=r), _sw(264, 136, 320, 1, r=r)]
        cs += [_rp(8, 256, 2, 2, 1, bias=0, r=r, qkv_cols=(256, 256)), _rp(264, 320, 4, 2, 1, r=r, qkv_cols=(512, 256)),
               _rp(37, 256, 2, 0, 1, r=r, qkv_cols=(256, 0))]
    # fallbacks (base GEMM rounded, + u Bl^T rounded again): K % 64 = 8; q_cols = 384 puts a block bound inside a tile
    cs += [_sw(264, 136, 264, 0, "exact256", r=8), _rp(264, 264, 4, 2, 0, "exact256", r=8, qkv_cols=(512, 256), bias=0),
           _rp(37, 256, 3, 1, 0, "exact256", r=8, qkv_cols=(384, 128))]
    cs += [_sw(264, 136, 320, 1, "gauss", r=8), _rp(264, 320, 4, 2, 1, "gauss", r=128, qkv_cols=(512, 256), bias=0)]
    names = [c.name for c in cs]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return cs


CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}


def is_multi(c):
    return c.M > 4000


def macs(c):
    return c.M * c.N * (c.K + c.r)


def entry(c):
    if c.op == "swiglu":
        return "vlr_gemm_swiglu_lora" if c.r else "vlr_gemm_swiglu"
    if c.op == "rope":
        return "vlr_gemm_qkv_rope_lora" if c.r else ("vlr_gemm_qkv_rope" if c.bias is None else "vlr_gemm_qkv_rope_bias")
    return "vlr_gemm_swiglu_bwd_add" if c.add else "vlr_gemm_swiglu_bwd"


def outputs(c):
    return {"swiglu": ("gu", "act"), "rope": ("qkv",), "bwd": ("gu", "ws")}[c.op]


def fused(c):
    return c.n256 == 1


# ---------------------------------------------------------------------------------------------------- operands
def guarded(rows, width, dtype, ld=None, data=None, behind=GUARD_ROWS, lead=0):
    """a NaN-filled flat buffer holding a logical [rows][width] matrix of row stride ld: GUARD + lead cells in front, `behind` more rows and
    GUARD cells at the end; data: the initial logical content"""
    ld = ld or width
    flat = torch.full((GUARD + lead + (rows + behind) * ld + GUARD,), NAN, dtype=dtype)
    b = Buf(flat, GUARD + lead, rows, width, ld)
    if data is not None:
        logical(b)[:] = data.reshape(rows, width)
    return b


def _values(c, shape, g, lim=8):
    if c.regime == "gauss":
        return torch.randn(*shape, generator=g) * 0.5
    if c.regime == "exact256":
        return torch.randint(-1, 2, shape, generator=g).float() * (torch.rand(*shape, generator=g) < 0.25)
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def positions(M, seed):
    """0 and MAX_POS - 1, a repeat, a descending step, -1, MAX_POS and 2^30 (clamped by both routes to [0, MAX_POS)) in the first eight
    rows; the out-of-range ones again around row 256 and in the last row; a descending run; random elsewhere"""
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(0, MAX_POS, (M,), generator=g)
    p[:8] = torch.tensor([0, MAX_POS - 1, 7, 7, 6, -1, MAX_POS, 2 ** 30])
    if M > 8:
        p[M - 1] = 2 ** 30
    if M > 258:
        p[254:258] = torch.tensor([MAX_POS, -1, 2 ** 30, -5])
        p[100:100 + MAX_POS] = torch.arange(MAX_POS - 1, -1, -1)
    return p.to(torch.int32)


_PLANTED = torch.tensor([0.0, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 0.0, 1.0, 0.5])


def planted_tables(half, max_pos=MAX_POS):
    """cos / sin [max_pos][half] fp32 with entries of _PLANTED by a hash of (table, position, feature)"""
    p = torch.arange(max_pos, dtype=torch.int64)[:, None]
    f = torch.arange(half, dtype=torch.int64)[None, :]
    out = []
    for salt in (0x9E3779B1, 0x85EBCA77):
        h = (p * 73856093 + salt) ^ (f * 19349663 + (salt >> 3))
        h = (h ^ (h >> 13)) * 1274126177
        h = (h ^ (h >> 16)) & 0x7FFFFFFF
        out.append(_PLANTED[h % len(_PLANTED)].to(F32))
    return out


def head_scales(c, n_heads, g):
    """per head of hd columns: a bias that dwarfs the product, one that vanishes beside it, zero, or one of its size"""
    pick = torch.arange(n_heads) % 4
    if c.regime == "gauss":
        return torch.tensor([64.0, 2.0 ** -10, 0.0, 0.5])[pick]
    return torch.tensor([512.0, 1.0 / 16, 0.0, 1.0])[pick]


def make(c):
    """-> dict of Bufs (and `pos`, a plain int32 tensor); see the module docstring"""
    g = torch.Generator().manual_seed(c.seed)
    M, N, K = c.M, c.N, c.K
    scale = 2.0 ** -6 if c.regime == "exact" and c.op != "rope" else 1.0
    inp = {}
    if c.op == "bwd":
        inp["dy"] = guarded(M, K, BF16, data=(_values(c, (M, K), g) * scale).to(BF16))
        inp["W"] = guarded(K, N, BF16, data=_values(c, (K, N), g).to(BF16), behind=0)              # wdown [H][I]
        inp["gu"] = guarded(M, 2 * N, BF16, data=(torch.randn(M, 2 * N, generator=g) * 2).to(BF16))
        add = None
        if c.add:
            add = torch.randn(M, N, generator=g) if c.regime == "gauss" else torch.randint(-64, 65, (M, N), generator=g).float() / 16
            add = add.to(BF16)
        inp["ws"] = guarded(M, N, BF16, data=add if c.add == "alias" else None)
        if c.add == "sep":
            inp["add"] = guarded(M, N, BF16, data=add)
        units = 64 * K + 64 * 4                       # in units of 2^-6
    else:
        inp["x"] = guarded(M, K, BF16, ld=c.ldx, data=(_values(c, (M, K), g) * scale).to(BF16))
        inp["W"] = guarded(N, K, BF16, data=_values(c, (N, K), g).to(BF16), behind=0)
        units = 64 * (K + c.r)
        if c.r:
            nb = len(c.blocks)
            inp["u"] = guarded(M, nb * c.r, BF16, ld=c.ldu, data=(_values(c, (M, nb * c.r), g) * scale).to(BF16))
            inp["Bl"] = guarded(N, c.r, BF16, data=_values(c, (N, c.r), g).to(BF16), behind=0)
        if c.op == "swiglu":
            inp["gu"] = guarded(M, N, BF16)
            inp["act"] = guarded(M, c.I, BF16)
        else:
            half = c.hd // 2
            if c.bias is not None:
                sc = head_scales(c, N // c.hd, g).repeat_interleave(c.hd)
                b = torch.randn(N, generator=g) if c.regime == "gauss" else torch.randint(-64, 65, (N,), generator=g).float()
                if c.regime == "exact256":
                    b, sc = b.clamp(-1, 1), torch.ones(N)
                inp["bias"] = guarded(1, N, BF16, data=(b * sc).to(BF16), behind=0, lead=c.bias)
                units += 64 * 512
            cos, sin = planted_tables(half) if c.tables == "planted" else rope_tables_f32(MAX_POS, c.hd)
            inp["cos"] = guarded(MAX_POS, half, F32, data=cos, behind=0)
            inp["sin"] = guarded(MAX_POS, half, F32, data=sin, behind=0)
            inp["pos"] = positions(M, c.seed)
            inp["qkv"] = guarded(M, N, BF16)
            units *= 4 * (4 if c.bias is None else 64)   # the rotation: two terms of up to 2 |x|, in units of 1/4 (1/64 with the smallest bias)
    if c.regime != "gauss":
        assert units < 2 ** 24, c                     # sum of the |terms| per element: every fp32 partial sum is exact
    return inp


# ---------------------------------------------------------------------------------------------------- the formulas
def _lg(inp, k, dev, dt, rows=None):
    t = logical(inp[k]).to(dev)
    return (t if rows is None else t[rows.to(dev)]).to(dt)


def accum(c, inp, dt, dev="cpu", rows=None, want_mag=False):
    """(the accumulators [rows][N] in dtype dt: x W^T or dy Wdown, + u Bl^T block by block; without bias and addend,  sum of the |terms|)"""
    a = _lg(inp, "dy" if c.op == "bwd" else "x", dev, dt, rows)
    w = _lg(inp, "W", dev, dt)
    w = w if c.op == "bwd" else w.t()
    acc = a @ w
    mag = a.abs() @ w.abs() if want_mag else None
    if c.r:
        u, bl = _lg(inp, "u", dev, dt, rows), _lg(inp, "Bl", dev, dt)
        lo = 0
        for t, hi in enumerate(c.blocks):
            ut = u[:, t * c.r:(t + 1) * c.r]
            acc[:, lo:hi] += ut @ bl[lo:hi].t()
            if want_mag:
                mag[:, lo:hi] += ut.abs() @ bl[lo:hi].abs().t()
            lo = hi
    return acc, mag


def _round_base(c, inp, dt, dev, rows, bias=None):
    """the fallback's intermediate in dtype dt: the base product (+ bias) rounded to bf16, the adapter term added to that and rounded again"""
    base, _ = accum(Case(c, r=0), inp, dt, dev, rows)
    if bias is not None:
        base = base + bias
    base = base.to(BF16).to(dt)
    if c.r:
        full, _ = accum(c, inp, dt, dev, rows)
        only_base, _ = accum(Case(c, r=0), inp, dt, dev, rows)
        base = (base + (full - only_base)).to(BF16).to(dt)       # (exact256: every term is a small integer, the difference is exact)
    return base


def _sigmoid(g):
    return 1.0 / (1.0 + torch.exp(-g))


def swiglu_fwd(g, u):
    """-> (act, its arithmetic magnitude max(|act|, |silu(g)|), |silu(g)|)"""
    s = g * _sigmoid(g)
    o = s * u
    return o, torch.maximum(o.abs(), s.abs()), s.abs()


def swiglu_bwd(d, g, u):
    """-> (d gate, d up, |d dg / d D|, |d du / d D|, arithmetic magnitudes of d gate and d up as in row_ref.Swiglu)"""
    sg = _sigmoid(g)
    kg, ku = u * sg * (1 + g * (1 - sg)), g * sg
    return d * kg, d * ku, kg.abs(), ku.abs(), (d * u * sg).abs() * (1 + g.abs() * (1 + sg)), (d * ku).abs()


def clamp_pos(pos, rows=None):
    p = pos.long().clamp(0, MAX_POS - 1)
    return p if rows is None else p[rows]


def rotate(c, x, cs, sn, mag=None):
    """rotate-half on the first rope_cols columns of x [rows][N]; cs, sn [rows][hd / 2].  -> (y, |x1 c| + |x2 s| terms, cos / sin weighted mag)"""
    R, half = x.shape[0], c.hd // 2
    nh = c.rope_cols // c.hd
    y, arith = x.clone(), torch.zeros_like(x)
    prop = None if mag is None else mag.clone()
    if nh:
        h = x[:, :c.rope_cols].reshape(R, nh, c.hd)
        x1, x2, cc, ss = h[..., :half], h[..., half:], cs[:, None, :], sn[:, None, :]
        y[:, :c.rope_cols] = torch.cat([x1 * cc - x2 * ss, x2 * cc + x1 * ss], -1).reshape(R, c.rope_cols)
        arith[:, :c.rope_cols] = torch.cat([(x1 * cc).abs() + (x2 * ss).abs(), (x2 * cc).abs() + (x1 * ss).abs()], -1).reshape(R, c.rope_cols)
        if mag is not None:
            m = mag[:, :c.rope_cols].reshape(R, nh, c.hd)
            m1, m2 = m[..., :half], m[..., half:]
            prop[:, :c.rope_cols] = torch.cat([m1 * cc.abs() + m2 * ss.abs(), m2 * cc.abs() + m1 * ss.abs()], -1).reshape(R, c.rope_cols)
    return y, arith, prop


def coef(c):
    return (c.K + c.r + 6) * U_MFMA if c.regime == "gauss" else 0.0


def _exp_bits(val):
    v32 = val.to(F32)
    assert bool((v32.to(F64) == val).all())           # a multiple of 2^-6 (1/16 for RoPE) below 2^24 units: float64 -> fp32 is exact
    return Exp(v32, None, None, None)


def _tables(c, inp, dev, dt, rows):
    p = clamp_pos(inp["pos"], rows).to(dev)
    return logical(inp["cos"]).to(dev)[p].to(dt), logical(inp["sin"]).to(dev)[p].to(dt)


def compute(c, inp, dt, dev="cpu", rows=None):
    """{output: (value, bound magnitude or None)} in dtype dt, following the case's route.  dt = F64: the reference with its bound
    (bound = U_BF16 |value| + magnitude; None = bitwise); dt = F32: the emulation (the caller rounds to bf16)"""
    ref = dt == F64
    gauss = c.regime == "gauss"
    assert fused(c) or not gauss, c
    k = coef(c)
    R = c.M if rows is None else len(rows)
    nanlike = lambda w: torch.full((R, w), NAN, dtype=dt, device=dev)      # noqa: E731
    if c.op == "swiglu":
        I = c.I
        if fused(c):
            acc, mag = accum(c, inp, dt, dev, rows, want_mag=ref and gauss)
            gu_b = k * mag if ref and gauss else None
        else:
            acc, gu_b = _round_base(c, inp, dt, dev, rows), None
        G, U = acc[:, :I], acc[:, I:]
        o, am, sa = swiglu_fwd(G, U)
        ab = None
        if ref:
            ab = (4 * U_F32 + TOL["fwd"][1]) * am
            if gauss:
                ab = ab + k * (1.1 * U.abs() * mag[:, :I] + sa * mag[:, I:])
        out = {"act": (o, ab)}
        if c.store_gu or c.r:
            out["gu"] = (acc, gu_b)
        elif fused(c):
            out["gu"] = (nanlike(2 * I), None)          # store_gu = 0 on the fused route: gu keeps its content (fallback: scratch)
        return out
    if c.op == "rope":
        bias = _lg(inp, "bias", dev, dt) if c.bias is not None else None
        cs, sn = _tables(c, inp, dev, dt, rows)
        if fused(c):
            acc, mag = accum(c, inp, dt, dev, rows, want_mag=ref and gauss)
            if bias is not None:
                acc = acc + bias
                mag = mag + bias.abs() if mag is not None else None
        else:
            acc, mag = _round_base(c, inp, dt, dev, rows, bias), None
        y, arith, prop = rotate(c, acc, cs, sn, mag)
        return {"qkv": (y, k * prop + 4 * U_F32 * arith if ref and gauss else None)}
    # the SwiGLU backward
    I = c.I
    add = _lg(inp, "add" if c.add == "sep" else "ws", dev, dt, rows) if c.add else None
    gu0 = _lg(inp, "gu", dev, dt, rows)
    g, u = gu0[:, :I], gu0[:, I:]
    acc, mag = accum(c, inp, dt, dev, rows, want_mag=ref and gauss)
    if add is not None:
        acc = acc + add
        mag = mag + add.abs() if mag is not None else None
    if not fused(c):
        acc = acc.to(BF16).to(dt)                        # d act through dact_ws
    dg, du, kg, ku, mg, mu = swiglu_bwd(acc, g, u)
    b = None
    if ref:
        b = (6 * U_F32 + TOL["bwd"][1]) * torch.cat([mg, mu], 1)
        if gauss:
            b = b + k * torch.cat([mag * kg, mag * ku], 1)
    return {"gu": (torch.cat([dg, du], 1), b)}


def bitwise(c, name):
    """the outputs compared bit for bit in the exact regimes: gate | up, and the whole q | k | v + RoPE result"""
    return c.regime != "gauss" and (name == "qkv" or (name == "gu" and c.op == "swiglu"))


def expect(c, inp, dev="cpu", rows=None):
    out = {}
    for name, (val, b) in compute(c, inp, F64, dev, rows).items():
        if bool(torch.isnan(val).all()):
            out[name] = Exp(val.to(F32), None, None, None)                    # must still hold its NaN prefill
        elif bitwise(c, name):
            if c.regime == "exact256":
                acc, mag = accum(c, inp, F64, dev, rows, want_mag=True)
                assert float(mag.max()) + (1 if c.op == "rope" and c.bias is not None else 0) <= 256, c
            out[name] = _exp_bits(val)
        else:
            out[name] = Exp(val, b, U_BF16, 1.0)
    return out


def emulate(c, inp, rows=None):
    return {name: val.to(BF16) for name, (val, _) in compute(c, inp, F32, "cpu", rows).items()}


def sample(c):
    """rows for the host test: None when the case is small, else every 128-row tile edge (which includes the 256 ones), the corners and
    a few interior rows - with ALL columns, so every column edge is there"""
    return _edges(c.M) if is_multi(c) else None


def place(c, inp, name, out, rows=None):
    """-> (Buf, flat buffer after a call that wrote `out` into output `name`); for a sampled case a compact buffer of the sampled rows
    whose initial content is the sampled old content"""
    b = inp[name]
    if rows is not None:
        b = guarded(len(rows), b.width, b.flat.dtype, ld=b.ld, data=logical(b)[rows])
    f = b.flat.clone()
    logical(b, f)[:] = out.to(f.dtype)
    return b, f


def check_case(c, inp, after, exp):
    """after: {output buffer: flat tensor after the call}.  Outputs expect() names are checked cell by cell, bounds or bits, and outside
    the logical result; the scratch ones (dact_ws; gu of a fallback with store_gu = 0) outside the logical result only"""
    for name in outputs(c):
        if name in exp:
            check(f"{c.name} {name}", after[name], inp[name], exp[name])
        else:
            check_poison(f"{c.name} {name}", after[name], inp[name])


def worst(c, inp, after, exp):
    """{output: worst |error| / bound} of the outputs with a bound"""
    return {n: worst_ratio(after[n], inp[n], e) for n, e in exp.items() if e.rel is not None}


# ---------------------------------------------------------------------------------------------------- choose_peel, restated
def peel_tail256_best(M, tn, ncu=256, rmax=6):
    """choose_peel(M, N, tn, ., ., tail256 = true) of csrc/gemm.hip with its integer divisions: the tile rows it peels (always 0)"""
    tm = (M + 255) // 256
    peel = 0
    if tm * tn >= 2 * ncu:
        best = float((tm * tn + ncu - 1) // ncu)
        for r in range(1, rmax + 1):
            if tm - r < 2:
                break
            est = float(((tm - r) * tn + ncu - 1) // ncu) + 1.15 * float((r * tn + ncu - 1) // ncu)
            if est < best - 0.05:
                best, peel = est, r
    return peel


# ---------------------------------------------------------------------------------------------------- the activation allowances
def measure_tol():
    """worst |fp32 epilogue - float64 epilogue| / magnitude of the SwiGLU forward and backward over this module's cases: both take the
    float64 accumulators rounded to fp32 (so the accumulation itself, which coef covers, does not count), unrounded outputs"""
    worst_ = {"fwd": 0.0, "bwd": 0.0}
    for c in CASES:
        if c.op == "rope":
            continue
        inp, rows = make(c), sample(c)
        acc, _ = accum(c, inp, F64, "cpu", rows)
        if c.op == "bwd" and c.add:
            acc = acc + _lg(inp, "add" if c.add == "sep" else "ws", "cpu", F64, rows)
        a32 = acc.to(F32)
        a64 = a32.to(F64)
        if c.op == "swiglu":
            o64, m, _ = swiglu_fwd(a64[:, :c.I], a64[:, c.I:])
            o32, _, _ = swiglu_fwd(a32[:, :c.I], a32[:, c.I:])
            worst_["fwd"] = max(worst_["fwd"], float(((o32.to(F64) - o64).abs() / m.clamp_min(1e-300)).max()))
        else:
            gu = _lg(inp, "gu", "cpu", F32, rows)
            g, u = gu[:, :c.I], gu[:, c.I:]
            r64 = swiglu_bwd(a64, g.to(F64), u.to(F64))
            r32 = swiglu_bwd(a32, g, u)
            for i in (0, 1):
                worst_["bwd"] = max(worst_["bwd"], float(((r32[i].to(F64) - r64[i]).abs() / r64[4 + i].clamp_min(1e-300)).max()))
    return worst_


if __name__ == "__main__":
    print({k: (float(f"{v:.2g}"), float(f"{4 * v:.2g}")) for k, v in sorted(measure_tol().items())})
    print("choose_peel(tail256) peels", max(peel_tail256_best(M, tn, ncu, 6) for ncu in (64, 128, 240, 256) for tn in range(1, 120)
                                             for M in range(256, 40000, 128)), "tile rows at most")
