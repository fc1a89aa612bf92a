"""Reference, case table and checker inputs for the GEMM family of csrc/gemm.hip, csrc/gemm128p.hip and csrc/gemm256p.hip (plain module, no
pytest hooks; CPU only unless a device is named).  tests/test_gemm_checker_host.py runs the checker on the CPU, tests/test_hip_gemm_edges.py
runs the same cases on the GPU.  Buffers, the checker and its conventions are those of tests/row_ref.py.

  CASES                one Case per launch: entry point, layout (0 NT, 1 NN, 2 TN), M N K, lda ldb ldc ldr, the epilogue (bias, act 0/1/2,
                       res None / "bf16" / "f32", acc, f32, alpha), the data regime, the expected route
  make(c)              CPU operands: A, B, the residual and C as strided Bufs (leading dimension > logical width; padding and GUARD cells
                       hold NaN), the bias behind GUARD cells; C pre-filled with NaN, or with data where acc (or the in-place residual) is set
  expect(c, inp)       Exp: float64 torch.matmul + the epilogue formula of gemm128_epilogue.h, act(alpha acc + bias) + residual + C_old
  emulate(c, inp)      the same in torch fp32, rounded once to the output type
  PAIRS                the pairs of vlr_gemm_bf16_tn_pair (their two problems are Cases of group "pair")
  sample(c)            rows and columns (every 128 / 256 tile edge, the corners, a few others) for the host test of a large case

The two data regimes.
  exact   A, B uniform integers in [-4, 4], bias / residual / old C integers within +-64, alpha in {1, 0.5, 0.25}; make() asserts
          sum |a||b| + |bias| + |res| + |C0| < 2^24 per element, so every partial sum in every order is exact in fp32 and the expected
          output is the float64 formula rounded ONCE to bf16 by round-to-nearest-even (unrounded for an fp32 output): the comparison is
          BITWISE.  At K >= 4096 a third to a half of the results are not representable in bf16, exact ties among them: the one
          rounding and its tie rule are under test.  "exact256": sparse +-1 data, asserted |exact| <= 256, for paths that round twice
          by design (every intermediate is then exact in bf16 too).  act 0 only.
  gauss   randn * 0.5.  ELEMENTWISE |out - ref64| <= rel |ref| + coef mag; rel = 2^-8 for a bf16 output, 0 for an fp32 output (row_ref);
          mag = |alpha| |A|.|B| + |bias| + |res| + |C0| in float64; coef = (K + K2 + splits + 6) 2^-23: that many sequential fp32 additions
          at one ulp each.  2^-23 and not 2^-24 because the guides of this project do not document how the bf16 MFMA rounds its internal
          adds (a truncating adder loses up to one ulp per addition, a rounding one half).  act 1 (x fast_sigmoid(1.702 x)) and act 2
          (gelu) call __expf / erff and have no derivable bound: TOL holds the worst error of the fp32 emulation against the float64
          reference over this module's cases of that activation, measured on the CPU in units of mag, and 4x that as the allowance.
Nothing here is derived from a kernel's output.

The expected route (written down for 256 compute CUs; the GPU test checks it, a mismatch fails):
  uses_256p   the launch reaches gemm256p_kernel (kernel id 5 of the in-library profiler)
  split_k     a slice kernel wrote fp32 partials into the registered split-K workspace (then splitk_reduce_kernel ran)
  peel_rows   vlr_gemm_peel_rows(M, N): the last rows the 256 + 128 pair gives to the 128 x 128 kernel
"""
import torch

from tests.row_ref import padded, logical, check, check_poison, worst_ratio, Exp, Buf, GUARD, U_BF16      # noqa: F401 (re-exported)

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
U_MFMA = 2.0 ** -23
LAYOUTS = ("nt", "nn", "tn")
DEVICE_REF_MACS = 10 ** 9          # above this many multiply-adds the GPU test computes the float64 reference on the device

# (measured worst |fp32 emulation - float64 reference| / mag over this module's cases of the activation, allowance = 4x measured).
# Obtained with `python -m tests.gemm_ref` (measure_tol() below, CPU).
TOL = {1: (1.4e-7, 5.7e-7), 2: (1.4e-7, 5.4e-7)}


class Case(dict):
    __getattr__ = dict.__getitem__

    def __repr__(self):
        return self["name"]


def _c(group, M, N, K, route, layout=0, regime="exact", tag="", bias=0, act=0, res=None, acc=0, f32=0, alpha=1.0, pad=8, inplace=0,
       splits=0, comm_cus=-1, sched=-1, ws_bytes=64 << 20, seed=None, groups=1, r=0, entry=None):
    """pad: elements every leading dimension exceeds its logical width by (the smallest the 16-byte accesses of the ring / 256 kernels
    allow is 8; the register-staged kernel's k-strided loads allow 4); ws_bytes: the split-K workspace the test registers"""
    a_w = M if layout == 2 else K
    b_w = K if layout == 0 else N
    entry = entry or ("f32res" if res == "f32" and not (bias or act or acc) else ("scaled" if alpha != 1.0 else "bf16"))
    assert res != "f32" or f32
    name = f"{group}-{LAYOUTS[layout]}-{M}x{N}x{K}-{regime}" + (f"-{tag}" if tag else "")
    p8 = -(-pad // 8) * 8                           # k-contiguous operands and bf16 rows move in 16-byte pieces
    lora = entry.startswith("lora")                 # vlr_gemm_lora takes W [N][K] and lora_B [N][r] without a leading dimension
    return Case(name=name, group=group, entry=entry, layout=layout, M=M, N=N, K=K, lda=a_w + (pad if layout == 2 else p8),
                ldb=b_w + (0 if lora else p8 if layout == 0 else pad), ldc=groups * N + (pad if f32 else p8), ldr=N + (pad if f32 else p8),
                groups=groups, ldu=r + 2 * p8, bias=bias, act=act, res=res, acc=acc, f32=f32, alpha=alpha, regime=regime, inplace=inplace,
                splits=splits, K2=r,
                uses_256p=route[0], split_k=route[1], peel_rows=route[2], comm_cus=comm_cus, sched=sched, ws_bytes=ws_bytes,
                seed=seed if seed is not None else (M * 31 + N * 17 + K * 7 + layout) % 100003)


def _epilogues(group, M, N, K, route, layout=0, splits=0, **kw):
    """the full epilogue set: bias + bf16 residual + accumulate with alpha 0.5 and a LARGE padding (ldc, ldr = N + 1000); fp32 out +
    accumulate + bias; fp32 out + fp32 residual in place and not in place (vlr_gemm_bf16_f32res)"""
    return [_c(group, M, N, K, route, layout, tag="bias-res-acc-a0.5", bias=1, res="bf16", acc=1, alpha=0.5, pad=1000, splits=splits, **kw),
            _c(group, M, N, K, route, layout, tag="f32-acc-bias", bias=1, acc=1, f32=1, splits=splits, **kw),
            _c(group, M, N, K, route, layout, tag="f32res-inplace", res="f32", f32=1, inplace=1, splits=splits, **kw),
            _c(group, M, N, K, route, layout, tag="f32res", res="f32", f32=1, splits=splits, **kw)]


def _gauss(group, M, N, K, route, layout=0, splits=0, acts=(0, 1, 2), **kw):
    return [_c(group, M, N, K, route, layout, regime="gauss", tag=f"act{a}" + ("-bias" if a else ""), act=a, bias=1 if a else 0, splits=splits, **kw)
            for a in acts]


R128 = (False, False, 0)
RSPLIT = (False, True, 0)
R256 = (True, False, 0)


def _build_cases():
    cs = []
    # ---- the LDS-DMA ring 128 x 128 kernel (every operand 16-byte aligned, few tiles, short K)
    for M, N, K in ((8, 8, 8), (128, 128, 64), (136, 136, 72), (200, 136, 72), (120, 248, 200)):
        cs += [_c("ring", M, N, K, R128, lay) for lay in range(3)]
    cs += _epilogues("ring", 200, 136, 72, R128) + _gauss("ring", 120, 248, 200, R128)
    # ---- the register-staged 128 x 128 kernel: operands the ring refuses (a k-strided operand whose width is no multiple of 8)
    cs += [_c("staged", 132, 136, 200, R128, 2, pad=4)]
    cs += [_c("staged", 136, 132, 72, R128, lay, f32=1, pad=4, tag="f32") for lay in (1, 2)]
    cs += [_c("staged", 136, 132, 72, R128, 1, f32=1, pad=4, tag="f32res", res="f32")]
    cs += _gauss("staged", 132, 136, 200, R128, 2, pad=4, acts=(0,))
    # ---- TN split-K (K >= 2048): 8 slices of 256; a last slice of 8 elements; of one K tile; the 16-slice cap; the workspace cap (3 slices)
    cs += [_c("tnsplit", 256, 64, 2048, RSPLIT, 2, splits=8), _c("tnsplit", 256, 64, 2248, RSPLIT, 2, splits=8),
           _c("tnsplit", 256, 64, 2624, RSPLIT, 2, splits=9), _c("tnsplit", 256, 64, 4096, RSPLIT, 2, splits=16),
           _c("tnsplit", 256, 64, 2048, RSPLIT, 2, splits=3, tag="ws-cap", ws_bytes=2 * 200704)]
    cs += _epilogues("tnsplit", 256, 64, 2248, RSPLIT, 2, splits=8) + _gauss("tnsplit", 256, 64, 2248, RSPLIT, 2, splits=8)
    # ---- skinny split-K (N <= 512, M >= 2048, K >= 2048), NT and NN
    for lay in (0, 1):
        cs += [_c("skinny", 2048, 128, 2048, RSPLIT, lay, splits=8), _c("skinny", 2056, 136, 2120, RSPLIT, lay, splits=7)]
    cs += _epilogues("skinny", 2056, 136, 2120, RSPLIT, splits=7) + _gauss("skinny", 2056, 136, 2120, RSPLIT, splits=7)
    # ---- general split-K (K >= 4096, fewer than 256 tiles of 128): everything through splitk_reduce_kernel
    cs += [_c("gensplit", 300, 264, 4096, RSPLIT, lay, splits=16) for lay in (0, 1)]
    cs += [_c("gensplit", 300, 264, 4096, RSPLIT, 0, splits=16, tag="acc", acc=1)]          # bf16 out, accumulate, ldc > N
    cs += _epilogues("gensplit", 300, 264, 4096, RSPLIT, splits=16) + _gauss("gensplit", 300, 264, 4096, RSPLIT, splits=16)
    # ---- per-tile 256 x 256 kernel, one tile per workgroup (192 .. 256 tiles): 12 x 16 tiles, and 12 x 17 with an 8-row last tile row
    # and an 8-column last tile column
    for M, N in ((3072, 4096), (2824, 4104)):
        cs += [_c("tile256", M, N, K, R256) for K in (64, 72, 192, 328)]
    cs += [_c("tile256", 2824, 4104, 72, R256, lay) for lay in (1, 2)]
    cs += _epilogues("tile256", 2824, 4104, 72, R256) + _gauss("tile256", 2824, 4104, 72, R256)
    # ---- per-tile 256 x 256 kernel, persistent (more than 256 tiles; K < 256 or an epilogue keeps it off the continuous pipeline)
    cs += [_c("pers256", 4104, 4104, 72, R256), _c("pers256", 4104, 4104, 320, R256, tag="bias", bias=1)]
    cs += [_c("pers256", 4104, 4104, 72, R256, lay) for lay in (1, 2)]
    cs += _epilogues("pers256", 4104, 4104, 72, R256) + _gauss("pers256", 4104, 4104, 72, R256)
    # ---- the continuous pipeline: its minimum K, its first tail, five K tiles; fp32 out + fp32 residual; uneven piece lists; the schedules
    cs += [_c("cont", 4104, 4104, K, R256) for K in (256, 264, 320)]
    cs += [_c("cont", 4104, 4104, 264, R256, lay) for lay in (1, 2)]
    cs += [_c("cont", 4104, 4104, 264, R256, tag="f32res-inplace", res="f32", f32=1, inplace=1),
           _c("cont", 4104, 4104, 264, R256, tag="f32res", res="f32", f32=1)]
    cs += [_c("cont", 2824, 4104, 256, R256, tag="comm128", comm_cus=128)]
    cs += [_c("cont", 4104, 4104, 320, R256, tag=f"sched{s}", sched=s) for s in (0, 16, 32)]
    cs += _gauss("cont", 4104, 4104, 264, R256, acts=(0,))
    # ---- the 256 + 128 peeled pair: 33 x 16 tiles, choose_peel gives the last 136 rows to the 128 kernel (un-split at K = 256, split at 4096)
    RP, RPS = (True, False, 136), (True, True, 136)
    cs += [_c("peel", 8328, 4096, 256, RP, lay) for lay in (0, 1)]
    cs += [_c("peel", 8328, 4096, 4096, RPS, splits=8)] + _epilogues("peel", 8328, 4096, 4096, RPS, splits=8)
    # ---- vlr_gemm_grouped, unmasked: groups of [136 x 136] whose outputs are column blocks of ONE buffer (gC = N), un-split (K < 1024)
    # and split along K (8 slices, reduced with gridDim.y = groups)
    for lay in (0, 2):
        for ng in (1, 3, 8):
            for K, sp in ((200, 0), (2048, 8)):
                cs += [_c("grouped", 136, 136, K, RSPLIT if sp else R128, lay, tag=f"g{ng}-acc{acc}", groups=ng, acc=acc, alpha=0.5, splits=sp,
                          entry="grouped") for acc in (0, 1)]
    cs += [_c("grouped", 136, 136, 2048, RSPLIT, 0, regime="gauss", tag="g3-acc1", groups=3, acc=1, alpha=0.5, splits=8, entry="grouped")]
    # ---- vlr_gemm_lora / vlr_gemm_lora_f32res: the adapter segment u . lora_B^T rides the K loop of the continuous pipeline (u a column
    # block of a wider buffer: ldu = r + 16); K % 64 != 0: the base GEMM (rounded) + seg_fallback_add (rounded again): the <= 256 data
    for res, f32, e in ((None, 0, "lora"), ("bf16", 0, "lora"), ("f32", 1, "lora_f32res")):
        t = f"r16-res{res}"
        cs += [_c("lora", 300, 256, 256, R256, tag=t, r=16, res=res, f32=f32, entry=e)]
        cs += [_c("lora", 300, 256, 264, R128, regime="exact256", tag=t, r=16, res=res, f32=f32, entry=e)]
    cs += [_c("lora", 4104, 4104, 256, R256, tag="r8-resbf16", r=8, res="bf16", entry="lora"),
           _c("lora", 4104, 4104, 256, R256, tag="r128-resbf16", r=128, res="bf16", entry="lora"),
           _c("lora", 4104, 4104, 256, R256, tag="r128-resf32", r=128, res="f32", f32=1, entry="lora_f32res"),
           _c("lora", 300, 256, 256, R256, regime="gauss", tag="r16-resbf16", r=16, res="bf16", entry="lora"),
           _c("lora", 4104, 4104, 256, R256, regime="gauss", tag="r128-resf32", r=128, res="f32", f32=1, entry="lora_f32res")]
    # ---- vlr_gemm_bf16_tn_pair: the two problems of each pair (PAIRS below)
    for pr in _PAIR_SHAPES:
        cs += [_c("pair", M, N, pr[3], R256 if pr[5] else R128, 2, tag=f"{pr[0]}-{i}", acc=pr[4], seed=1000 + 7 * i + len(cs))
               for i, (M, N) in enumerate(pr[1:3])]
    names = [c.name for c in cs]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return cs


# (name, (M0, N0), (M1, N1), K, accumulate, joint).  tn_pair_plan on 256 CUs: the joint launch needs at least a quarter of a round saved
# and, AFTER the tile rows the plan gives to the 128 kernel, still more than 256 tiles of 256 (17 x 16 + 1 tiles do not qualify: the plan
# peels two tile rows, 241 tiles remain, the launch declines and two single calls run).  20 x 13 + 3 x 12 = 296 tiles, 2 rounds instead of
# 2 + 1 and nothing peeled, is the smallest pair of sizes 8 over a tile edge that takes it.  17 x 16 + 16 x 16 = 528 tiles: 3 rounds
# either way, but with the last tile row (8 rows) of problem 0 on the 128 kernel 512 tiles = 2 rounds + 0.7.
# accumulate = 1 is never joint; 256 + 256 tiles are 2 rounds together and apart.
_PAIR_SHAPES = [("joint-smallest", (4872, 3080), (520, 2824), 256, 0, True), ("joint-peel", (4104, 4096), (4096, 4096), 256, 0, True),
                ("fallback-acc", (136, 136), (200, 136), 72, 1, False), ("fallback-equal-rounds", (4096, 4096), (4096, 4096), 64, 0, False)]
CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}
PAIRS = [Case(name=n, cases=tuple(c for c in CASES if c.group == "pair" and f"-{n}-" in c.name), K=K, acc=acc, joint=joint)
         for n, _, _, K, acc, joint in _PAIR_SHAPES]
assert all(len(p.cases) == 2 for p in PAIRS)
RING_SUBSET = [c for c in CASES if c.group == "ring"]      # run again on the register-staged kernel (VLR_GEMM128P=0, a child process)


def row_bits(t):
    """the tensor's bit patterns (NaN cells compare equal to themselves)"""
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def macs(c):
    return c.groups * c.M * c.N * (c.K + c.K2)


# ---------------------------------------------------------------------------------------------------- operands
def _values(c, shape, gen, lim):
    if c.regime == "gauss":
        return torch.randn(*shape, generator=gen) * 0.5
    if c.regime == "exact256":
        return torch.randint(-1, 2, shape, generator=gen).float() * (torch.rand(*shape, generator=gen) < 0.25)
    return torch.randint(-lim, lim + 1, shape, generator=gen).float()


def make(c):
    """-> dict(A, B, C: Buf; R: Buf or None (None too when the residual IS C: inplace); bias: Buf or None)"""
    g = torch.Generator().manual_seed(c.seed)
    ng = c.groups                                   # grouped: the groups' operands stacked along the rows, their outputs side by side
    a_shape = (ng * c.K, c.M) if c.layout == 2 else (ng * c.M, c.K)
    b_shape = (ng * c.N, c.K) if c.layout == 0 else (ng * c.K, c.N)
    A = padded(*a_shape, BF16, ld=c.lda, data=_values(c, a_shape, g, 4).to(BF16))
    B = padded(*b_shape, BF16, ld=c.ldb, data=_values(c, b_shape, g, 4).to(BF16))
    odt = F32 if c.f32 else BF16
    bias = padded(1, c.N, BF16, data=_values(c, (1, c.N), g, 64).to(BF16)) if c.bias else None
    res = _values(c, (c.M, c.N), g, 64).to(F32 if c.res == "f32" else BF16) if c.res else None
    c0 = _values(c, (c.M, ng * c.N), g, 64).to(odt) if c.acc else None
    if c.inplace:
        assert c.res == "f32" and c.f32 and not c.acc
        Cb, Rb = padded(c.M, c.N, odt, ld=c.ldc, data=res), None
    else:
        Cb = padded(c.M, ng * c.N, odt, ld=c.ldc, data=c0)
        Rb = padded(c.M, c.N, res.dtype, ld=c.ldr, data=res) if c.res else None
    inp = dict(A=A, B=B, C=Cb, R=Rb, bias=bias, U=None, Bl=None)
    if c.K2:
        inp["U"] = padded(c.M, c.K2, BF16, ld=c.ldu, data=_values(c, (c.M, c.K2), g, 4).to(BF16))
        inp["Bl"] = padded(c.N, c.K2, BF16, data=_values(c, (c.N, c.K2), g, 4).to(BF16))
    if c.regime != "gauss":
        assert c.act == 0 and c.alpha in (1.0, 0.5, 0.25), c
        top = 16 * (c.K + c.K2) + 64 * (bool(c.bias) + bool(c.res) + bool(c.acc))
        assert top < 2 ** 24, c                         # sum |a||b| + |bias| + |res| + |C0| per element: every fp32 partial sum is exact
    return inp


def _ab(c, inp, dt, dev, rows=None, cols=None):
    """[groups][M][K], [groups][N][K]"""
    a = logical(inp["A"]).to(dev).reshape(c.groups, -1, inp["A"].width)
    b = logical(inp["B"]).to(dev).reshape(c.groups, -1, inp["B"].width)
    a = a.transpose(1, 2) if c.layout == 2 else a
    b = b if c.layout == 0 else b.transpose(1, 2)
    if rows is not None:
        assert c.groups == 1
        a, b = a[:, rows], b[:, cols]
    return a.to(dt), b.to(dt)


def _side_by_side(x):
    """[groups][M][N] -> [M][groups N]"""
    return x.permute(1, 0, 2).reshape(x.shape[1], -1)


def _sub(t, rows, cols):
    return t if rows is None else t[rows][:, cols]


def _act(x, act):
    if act == 1:
        return x / (1.0 + torch.exp(-1.702 * x))
    if act == 2:
        return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752))
    return x


def formula(c, inp, dt, dev="cpu", rows=None, cols=None):
    """(value, mag) of act(alpha A.B + bias) + residual + C_old in dtype dt on device dev, of the whole result or of rows x cols"""
    a, b = _ab(c, inp, dt, dev, rows, cols)
    want_mag = dt == F64 and c.regime != "exact"
    x = c.alpha * _side_by_side(a @ b.transpose(1, 2))
    mag = abs(c.alpha) * _side_by_side(a.abs() @ b.abs().transpose(1, 2)) if want_mag else None
    if c.K2:
        u, bl = logical(inp["U"]).to(dev).to(dt), logical(inp["Bl"]).to(dev).to(dt)
        if rows is not None:
            u, bl = u[rows], bl[cols]
        x = x + u @ bl.t()
        mag = mag + u.abs() @ bl.abs().t() if want_mag else None
    if c.bias:
        bv = logical(inp["bias"]).to(dev).to(dt)
        bv = bv if cols is None else bv[:, cols]
        x = x + bv
        mag = mag + bv.abs() if mag is not None else None
    x = _act(x, c.act)
    for on, buf in ((c.res, inp["C"] if c.inplace else inp["R"]), (c.acc, inp["C"])):
        if on:
            t = _sub(logical(buf).to(dev), rows, cols).to(dt)
            x = x + t
            mag = mag + t.abs() if mag is not None else None
    return x, mag


def coef(c):
    return (c.K + c.K2 + c.splits + 6) * U_MFMA + (TOL[c.act][1] if c.act else 0.0)


def expect(c, inp, dev="cpu", rows=None, cols=None):
    val, mag = formula(c, inp, F64, dev, rows, cols)
    if c.regime == "gauss":
        return Exp(val, mag, 0.0 if c.f32 else U_BF16, coef(c))
    if c.regime == "exact256":
        assert float(mag.max()) <= 256, c              # the sum of the |terms|: every intermediate in every order is an integer <= 256
    # exact: val is an integer multiple of 1/4 below 2^24, so float64 -> float32 is exact and -> bf16 rounds once, to nearest even
    return Exp(val.to(F32), None, None, None)


def emulate(c, inp, rows=None, cols=None, unrounded=False):
    val, _ = formula(c, inp, F32, "cpu", rows, cols)
    return val if unrounded else val.to(F32 if c.f32 else BF16)


def _edges(n, tile=128):
    s = {0, 1, n - 1, n - 2, n // 2, n // 3}
    for e in range(tile, n, tile):
        s.update((e - 1, e, e + 1))
    return torch.tensor(sorted(i for i in s if 0 <= i < n))


def sample(c):
    """(rows, cols) for the host test: None, None when the case is small; else every 128-tile edge (which includes the 256 ones), the
    corners and a few interior rows / columns"""
    if macs(c) <= 4 * 10 ** 8:
        return None, None
    return _edges(c.M), _edges(c.N)


def place(c, inp, out, rows=None, cols=None):
    """-> (Buf, flat buffer after a call that wrote `out`): C's own buffer, or for a sampled case a compact buffer of the sampled shape
    whose initial content is the sampled old C"""
    if rows is None:
        b = inp["C"]
    else:
        old = _sub(logical(inp["C"]), rows, cols)
        b = padded(len(rows), len(cols), old.dtype, ld=len(cols) + 8, data=old)
    f = b.flat.clone()
    logical(b, f)[:] = out.to(f.dtype)
    return b, f


def alignment_errors(c):
    """why the entry point would refuse the case (the VLR_REQUIREs of gemm_impl_ex, gemm_grouped, gemm_lora_impl); empty: it takes it"""
    bad = []
    if c.entry == "grouped" and (c.N % 8 or c.lda % 8 or c.ldb % 8 or c.ldc % 8 or c.f32 or c.bias or c.res or c.act or c.layout == 1):
        bad.append("grouped")
    if c.K2 and (c.layout or c.K2 % 8 or c.ldu % 8 or c.ldu < c.K2 or c.ldb != c.K or c.lda % 8 or c.ldc % 8 or c.N % 8 or c.K % 8 or c.bias
                 or c.act or c.acc or c.alpha != 1.0 or (c.res == "f32") != bool(c.f32 and c.res) or (c.f32 != (c.entry == "lora_f32res"))):
        bad.append("lora")
    if c.group == "pair" and (c.layout != 2 or c.bias or c.res or c.act or c.f32 or c.alpha != 1.0):
        bad.append("pair")
    a_ks, b_ks = c.layout == 2, c.layout != 0
    if a_ks and (c.lda % 4 or c.M % 4) or not a_ks and (c.lda % 8 or c.K % 8):
        bad.append("A")
    if b_ks and (c.ldb % 4 or c.N % 4) or not b_ks and (c.ldb % 8 or c.K % 8):
        bad.append("B")
    q = 4 if c.f32 else 8
    if c.N % q or c.ldc % q:
        bad.append("C")
    if c.res and (c.ldc if c.inplace else c.ldr) % q:
        bad.append("residual")
    if c.res == "f32" and not c.f32:
        bad.append("fp32 residual needs fp32 out")
    if c.entry == "f32res" and (c.bias or c.act or c.acc or c.alpha != 1.0):
        bad.append("f32res epilogue")
    if c.lda < (c.M if a_ks else c.K) or c.ldb < (c.N if b_ks else c.K) or c.ldc < c.groups * c.N or c.ldr < c.N:
        bad.append("ld below width")
    return bad


def measure_tol():
    """worst |unrounded fp32 emulation - float64 reference| / mag per activation over this module's gauss cases (how TOL was obtained)"""
    worst = {}
    for c in CASES:
        if not c.act:
            continue
        inp = make(c)
        rows, cols = sample(c)
        val, mag = formula(c, inp, F64, "cpu", rows, cols)
        emu = emulate(c, inp, rows, cols, unrounded=True)
        worst[c.act] = max(worst.get(c.act, 0.0), float(((emu.to(F64) - val).abs() / mag.clamp_min(1e-300)).max()))
    return worst


if __name__ == "__main__":
    print({a: (float(f"{v:.2g}"), float(f"{4 * v:.2g}")) for a, v in sorted(measure_tol().items())})
