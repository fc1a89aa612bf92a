"""References, case tables and checkers for the row / reduction / loss / optimizer kernels of csrc/elementwise.hip and csrc/dpo_ops.hip
(plain module, no pytest hooks; CPU only).  tests/test_row_checker_host.py runs the checkers on the CPU, tests/test_hip_row_edges.py
runs the same cases on the GPU.

  OPS[name]            one Op per entry point: .cases (the issue's shapes, names usable as pytest ids), .make(c) -> CPU inputs (the bf16 /
                       fp32 tensors the kernel gets, strided ones with NaN past the logical width), .formula(c, inp, dt) -> the operation
                       in dtype dt (float64 = the reference, float32 = the emulation), .exact(c, inp) -> integer / copy outputs,
                       .buffers(c, inp) -> the padded, poisoned output buffers, .geom(c) -> where its loops end
  expect(op, c, inp)   {output: Exp}: float64 reference, sum of |terms|, the bound's two coefficients
  emulate_fp32(...)    the same formula in torch fp32 (kernel order where it is stated), rounded once to the output type
  check(...)           ELEMENTWISE |out - ref| <= rel |ref| + coef mag, then: every cell outside the logical result is bit-identical to
                       what the buffer held before the call (NaN / integer poison, or the neighbouring data of an in-place operation)

The bound.  rel = 2^-8 for a bf16 output, 0 for an fp32 output: one round-to-nearest-even to bf16's 8-bit significand moves a value by
half an ulp, which is 2^-9 of it at the top of a binade and 2^-8 at the bottom - so 2^-8 |ref| admits ONE correct rounding and nothing
more (a result one bf16 ulp off fails everywhere).
coef = N 2^-24 + allowance.  N 2^-24 mag is the fp32 accumulation: N = the number of terms ONE accumulator adds (a thread's share of the
row, then 6 shuffle levels, then the waves' partials - n_acc()) plus the handful of roundings of the elementwise arithmetic around it;
mag = sum of |terms| = the float64 formula with every term replaced by its absolute value (each formula returns it next to the value).
For a pure elementwise operation N = 4 (2^-22 of the largest intermediate).  allowance: kernels that call __expf, rsqrtf, v_rcp_f32, erff
or logf have no derivable bound; TOL holds, per operation and output, the worst error of the fp32 emulation against the float64
reference over the operation's cases, in units of mag, measured on the CPU, and 4x that as the allowance (the 1-2 ulp hardware
intrinsics the emulation does not model).  Nothing here is derived from a kernel's output.
"""
import math
from collections import namedtuple

import numpy as np
import torch

from oracle import llava_dpo_oracle as O

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
U_BF16 = 2.0 ** -8          # half a bf16 ulp at the bottom of a binade
U_F32 = 2.0 ** -24
GUARD = 16                  # poison cells in front of and behind every output buffer (16 elements: the logical result stays 16-byte aligned)
SEAM = 4096 * 256           # grid_for(): 4096 workgroups of 256 threads, then the grid-stride loop
INT_POISON = {torch.int32: -7777777, torch.int64: -7777777, torch.uint8: 0xA5}

Exp = namedtuple("Exp", "ref mag rel coef")        # rel None: exact (bitwise; NaN must stay NaN)
Buf = namedtuple("Buf", "flat off rows width ld")  # logical [rows][width] at flat[off + r * ld + c]

# (measured worst |emulation - reference| / mag over the operation's cases, allowance = 4x measured); see the module docstring.
# Obtained with `python -m tests.row_ref` (measure_tol() below: the unrounded fp32 emulation against the float64 reference, CPU).
TOL = {
    "rmsnorm_fwd": {"y": (1.8e-7, 7.2e-7), "rstd": (7.2e-8, 2.9e-7)},
    "rmsnorm_fwd_f32": {"y": (2.0e-7, 8.2e-7), "rstd": (9.5e-8, 3.8e-7)},
    "layernorm_fwd": {"y": (1.6e-7, 6.5e-7)},
    "vit_embed_ln": {"y": (1.4e-7, 5.6e-7)},
    "layernorm_bwd": {"dx": (1.7e-7, 6.9e-7), "dw": (6.6e-8, 2.6e-7)},
    "swiglu_fwd": {"act": (2.1e-7, 8.6e-7)},
    "swiglu_bwd": {"gu": (2.3e-7, 9.3e-7)},
    "gelu_fwd": {"h": (1.1e-7, 4.4e-7)},
    "gelu_bwd": {"dz": (1.7e-7, 7.0e-7)},
    "logp_rows": {"lse": (5.9e-8, 2.4e-7), "tok": (7.0e-8, 2.8e-7)},
    "dlogits_rows": {"dl": (6.1e-8, 2.5e-7)},
}


class Case(dict):
    __getattr__ = dict.__getitem__

    def __repr__(self):
        return self["name"]


def _case(name, **kw):
    return Case(name=name, **kw)


def n_acc(total, lanes=256):
    """terms one accumulator adds when `lanes` threads share `total` terms: its own share, 6 shuffle levels, the waves' partials"""
    return -(-total // lanes) + 6 + max(1, lanes // 64)


def rnd(*shape, seed=0, scale=1.0, dtype=BF16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


# ---------------------------------------------------------------------------------------------------- buffers and the checker
def padded(rows, width, dtype, ld=None, data=None):
    """a poisoned flat buffer holding a logical [rows][width] matrix of row stride ld behind GUARD cells; data: initial logical content
    (in-place operations, accumulate)"""
    ld = ld or width
    n = GUARD + rows * ld + GUARD
    if dtype.is_floating_point:
        flat = torch.full((n,), float("nan"), dtype=dtype)
    else:
        flat = torch.full((n,), INT_POISON[dtype], dtype=dtype)
    b = Buf(flat, GUARD, rows, width, ld)
    if data is not None:
        logical(b)[:] = data.reshape(rows, width)
    return b


def logical(b, flat=None):
    """the [rows][width] view of the logical result inside b (or inside another flat tensor of b's layout)"""
    flat = b.flat if flat is None else flat
    return flat[b.off:b.off + b.rows * b.ld].view(b.rows, b.ld)[:, :b.width]


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def check_poison(what, after, b):
    """every cell of `after` outside b's logical result is bit-identical to b.flat (the content before the call)"""
    out = torch.ones(b.flat.numel(), dtype=torch.bool)
    logical(b, out)[:] = False
    bad = out & (_bits(after) != _bits(b.flat))
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: cell {i - b.off} of the buffer (outside the {b.rows} x {b.width} result, ld {b.ld}) was overwritten "
                             f"({int(bad.sum())} such cells)")


def check(what, after, b, e):
    """after: the whole flat buffer after the call (CPU); b: its Buf as made before the call; e: Exp"""
    assert after.shape == b.flat.shape and after.dtype == b.flat.dtype, what
    out = logical(b, after)
    ref = e.ref.reshape(b.rows, b.width)
    if e.rel is None:
        if out.dtype.is_floating_point:
            nan = torch.isnan(ref)
            ok = torch.where(nan, torch.isnan(out), _bits(out.contiguous()) == _bits(ref.to(out.dtype).contiguous()))
        else:
            ok = out == ref.to(out.dtype)
        if not bool(ok.all()):
            r, c = (~ok).nonzero()[0].tolist()
            raise AssertionError(f"{what}: [{r}][{c}] = {out[r, c].item()!r}, expected exactly {ref[r, c].item()!r} ({int((~ok).sum())} cells differ)")
    else:
        x = out.to(F64)
        bound = e.rel * ref.abs() + e.coef * e.mag.reshape(b.rows, b.width)
        err = (x - ref).abs()
        bad = ~(err <= bound)                        # NaN / inf in the output fail
        if bool(bad.any()):
            over = torch.where(bad, torch.nan_to_num(err / bound.clamp_min(1e-300), nan=math.inf, posinf=math.inf), torch.zeros_like(err))
            r, c = (over == over.max()).nonzero()[0].tolist()
            raise AssertionError(f"{what}: [{r}][{c}] = {x[r, c].item():.9g}, reference {ref[r, c].item():.9g}, |error| {err[r, c].item():.3e} > "
                                 f"bound {bound[r, c].item():.3e} ({int(bad.sum())} of {bad.numel()} elements out of bound)")
    check_poison(what, after, b)


def worst_ratio(after, b, e):
    """largest |out - ref| / bound over the logical result (measuring only; never used to set a bound)"""
    x, ref = logical(b, after).to(F64), e.ref.reshape(b.rows, b.width)
    bound = e.rel * ref.abs() + e.coef * e.mag.reshape(b.rows, b.width)
    return float(torch.nan_to_num((x - ref).abs() / bound.clamp_min(1e-300), nan=math.inf).max())


# ---------------------------------------------------------------------------------------------------- operations
class Op:
    name = ""
    kinds = {}            # output -> "bf16" | "f32" | "exact"
    cases = ()
    elementwise = False   # N = 4

    def make(self, c):
        raise NotImplementedError

    def formula(self, c, inp, dt):
        """{output: (value, mag, N)} in dtype dt"""
        return {}

    def exact(self, c, inp):
        return {}

    def emulate(self, c, inp):
        """unrounded fp32 outputs; default: the formula in fp32"""
        return {k: v[0] for k, v in self.formula(c, inp, F32).items()}

    def buffers(self, c, inp):
        raise NotImplementedError

    def geom(self, c):
        """output -> dict(pass_cols= columns one pass of the workgroup covers, seam= first flat element of the grid-stride loop,
        row_stride= rows one pass of the grid covers, width= columns the kernel writes when fewer than the logical result)"""
        return {}

    def seam_mask(self, c, name, b):
        """bool [rows][width]: the elements written by the second and later passes of the grid-stride loop (None: no such loop)"""
        seam = self.geom(c).get(name, {}).get("seam")
        if seam is None or seam >= b.rows * b.width:
            return None
        m = torch.zeros(b.rows * b.width, dtype=torch.bool)
        m[seam:] = True
        return m.view(b.rows, b.width)


OUT_DTYPE = {"bf16": BF16, "f32": F32}


def expect(op, c, inp):
    op = OPS[op] if isinstance(op, str) else op
    out = {}
    for k, (val, mag, n) in op.formula(c, inp, F64).items():
        kind = op.kinds[k]
        if isinstance(n, tuple):                     # (rtol, atol) taken over from an existing test
            out[k] = Exp(val, torch.ones_like(val), n[0], n[1])
            continue
        allow = TOL.get(op.name, {}).get(k, (0.0, 0.0))[1]
        out[k] = Exp(val, mag, U_BF16 if kind == "bf16" else 0.0, n * U_F32 + allow)
    for k, val in op.exact(c, inp).items():
        out[k] = Exp(val, None, None, None)
    return out


def emulate_fp32(op, c, inp):
    """{output: tensor of the kernel's output dtype}: fp32 arithmetic, rounded once"""
    op = OPS[op] if isinstance(op, str) else op
    out = {k: v.to(OUT_DTYPE[op.kinds[k]]) for k, v in op.emulate(c, inp).items()}
    out.update(op.exact(c, inp))
    return out


def _rms_terms(x, H, eps, dt):
    ss = (x * x).sum(-1, keepdim=True)
    return torch.rsqrt(ss / H + torch.tensor(eps, dtype=F32).to(dt))


class RmsnormFwd(Op):
    kinds = {"y": "bf16", "rstd": "f32"}

    def __init__(self, f32):
        self.name = "rmsnorm_fwd_f32" if f32 else "rmsnorm_fwd"
        self.f32 = f32
        self.cases = [_case(f"H{H}", M=3, H=H) for H in (8, 2048, 2056, 5120, 8192, 8200, 12288)]

    def make(self, c):
        return dict(x=rnd(c.M, c.H, seed=1, dtype=F32 if self.f32 else BF16), w=(1 + 0.1 * rnd(c.H, seed=2).float()).bfloat16(), eps=1e-5)

    def formula(self, c, inp, dt):
        x, w = inp["x"].to(dt), inp["w"].to(dt)
        rstd = _rms_terms(x, c.H, inp["eps"], dt)
        y = w * (x * rstd)
        n = n_acc(c.H) + 4
        return {"y": (y, y.abs(), n), "rstd": (rstd.reshape(-1), rstd.reshape(-1), n)}

    def buffers(self, c, inp):
        return {"y": padded(c.M, c.H, BF16), "rstd": padded(1, c.M, F32)}

    def geom(self, c):
        return {"y": dict(pass_cols=2048)}


class RmsnormBwd(Op):
    kinds = {"dx": "bf16", "dw": "bf16"}
    G = 1024

    def __init__(self, f32):
        self.name = "rmsnorm_bwd_f32" if f32 else "rmsnorm_bwd"
        self.f32 = f32
        self.cases = []
        for M, H in ((1, 8), (15, 4096), (16, 4104), (1024, 256), (1025, 5120), (2100, 8192)):
            variants = [(1, 1, 0), (1, 1, 1), (0, 1, 0), (1, 0, 0)] if (M, H) in ((16, 4104), (1025, 5120)) else [(1, 1, 1)]
            for dres, dw, acc in variants:
                self.cases.append(_case(f"M{M}-H{H}-dres{dres}-dw{dw}-acc{acc}", M=M, H=H, dres=dres, dw=dw, acc=acc))

    def make(self, c):
        x = rnd(c.M, c.H, seed=1, dtype=F32 if self.f32 else BF16)
        rstd = _rms_terms(x.to(F64), c.H, 1e-5, F64).reshape(-1).to(F32)         # an input of the backward: the forward's fp32 rstd
        return dict(x=x, w=(1 + 0.1 * rnd(c.H, seed=2).float()).bfloat16(), dy=rnd(c.M, c.H, seed=3), rstd=rstd,
                    dres=rnd(c.M, c.H, seed=4) if c.dres else None, dw0=rnd(c.H, seed=9))

    def formula(self, c, inp, dt):
        x, w, dy, rs = inp["x"].to(dt), inp["w"].to(dt), inp["dy"].to(dt), inp["rstd"].to(dt)[:, None]
        xh, gx = x * rs, dy * w
        dot = (gx * xh).sum(-1, keepdim=True) / c.H
        dx = rs * (gx - xh * dot)
        mdx = rs * (gx.abs() + xh.abs() * (gx * xh).abs().sum(-1, keepdim=True) / c.H)
        if inp["dres"] is not None:
            dx = dx + inp["dres"].to(dt)
            mdx = mdx + inp["dres"].to(dt).abs()
        out = {"dx": (dx, mdx, n_acc(c.H) + 6)}
        if c.dw:
            dw, mdw = (dy * xh).sum(0), (dy * xh).abs().sum(0)
            if c.acc:
                dw, mdw = dw + inp["dw0"].to(dt), mdw + inp["dw0"].to(dt).abs()
            out["dw"] = (dw, mdw, -(-c.M // self.G) + 64 + 16 + 4)               # rows per workgroup, then 1024 -> 16 -> 1
        return out

    def buffers(self, c, inp):
        b = {"dx": padded(c.M, c.H, BF16)}
        if c.dw:
            b["dw"] = padded(1, c.H, BF16, data=inp["dw0"])                      # without accumulate the old content must not matter
        return b

    def geom(self, c):
        return {"dx": dict(pass_cols=2048, row_stride=self.G), "dw": dict(row_stride=self.G)}

    reduction_outs = ("dw",)

    def drop_rows(self, c, inp, k):
        d = dict(inp)
        d["dy"] = inp["dy"].clone()
        d["dy"][c.M - k:] = 0
        return d

    def shift_pass(self, c, inp):
        if c.M <= self.G:
            return None
        d = dict(inp)
        hi = min(c.M - 1, 2 * self.G)
        for k in ("x", "dy", "rstd"):
            d[k] = inp[k].clone()
            d[k][self.G:hi] = inp[k][self.G + 1:hi + 1]
        return d


class LayernormFwd(Op):
    kinds = {"y": "bf16"}

    def __init__(self, embed):
        self.name = "vit_embed_ln" if embed else "layernorm_fwd"
        self.embed = embed
        self.cases = [_case(f"D{D}", M=6 if embed else 5, D=D, n_img=2, T=3) for D in (8, 1024, 1664, 2048, 2056, 4096)]

    def make(self, c):
        d = dict(w=rnd(c.D, seed=2), b=rnd(c.D, seed=3), eps=1e-5)
        if self.embed:
            d.update(pe=rnd(c.n_img * (c.T - 1), c.D, seed=4), cls=rnd(c.D, seed=5), pos=rnd(c.T, c.D, seed=6))
        else:
            d["x"] = rnd(c.M, c.D, seed=1) + 0.5
        return d

    def formula(self, c, inp, dt):
        if self.embed:
            pe, cls, pos = inp["pe"].to(dt), inp["cls"].to(dt), inp["pos"].to(dt)
            x = torch.cat([cls.expand(c.n_img, 1, c.D), pe.reshape(c.n_img, c.T - 1, c.D)], 1) + pos[None]
            x = x.reshape(c.n_img * c.T, c.D)
        else:
            x = inp["x"].to(dt)
        w, b = inp["w"].to(dt), inp["b"].to(dt)
        mean = x.sum(-1, keepdim=True) / c.D
        d = x - mean
        rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) / c.D + torch.tensor(inp["eps"], dtype=F32).to(dt))
        y = d * rstd * w + b
        mag = (x.abs() + x.abs().sum(-1, keepdim=True) / c.D) * rstd * w.abs() + b.abs()
        return {"y": (y, mag, 2 * n_acc(c.D) + 6)}

    def buffers(self, c, inp):
        return {"y": padded(c.M, c.D, BF16)}

    def geom(self, c):
        return {"y": dict(pass_cols=2048)}


class LayernormBwd(Op):
    name = "layernorm_bwd"
    kinds = {"dx": "bf16", "dw": "bf16", "db": "bf16"}
    G = 256
    reduction_outs = ("dw", "db")

    def __init__(self):
        self.cases = []
        for M, D in ((1, 8), (255, 2056), (256, 4096), (257, 2056), (600, 1664)):
            for dx, dwdb, acc in ((1, 1, 0), (0, 1, 0), (1, 0, 0), (1, 1, 1)):
                self.cases.append(_case(f"M{M}-D{D}-dx{dx}-dwdb{dwdb}-acc{acc}", M=M, D=D, dx=dx, dwdb=dwdb, acc=acc))

    def make(self, c):
        return dict(x=rnd(c.M, c.D, seed=1) + 0.5, w=rnd(c.D, seed=2), dy=rnd(c.M, c.D, seed=3), eps=1e-5, dw0=rnd(c.D, seed=7), db0=rnd(c.D, seed=8))

    def formula(self, c, inp, dt):
        x, w, dy = inp["x"].to(dt), inp["w"].to(dt), inp["dy"].to(dt)
        D = c.D
        mean = x.sum(-1, keepdim=True) / D
        d = x - mean
        rs = torch.rsqrt((d * d).sum(-1, keepdim=True) / D + torch.tensor(inp["eps"], dtype=F32).to(dt))
        xh, g = d * rs, dy * w
        xha = (x.abs() + x.abs().sum(-1, keepdim=True) / D) * rs
        sg, sgx = g.sum(-1, keepdim=True) / D, (g * xh).sum(-1, keepdim=True) / D
        out = {}
        nrow = 2 * n_acc(D) + 8
        if c.dx:
            mag = rs * (g.abs() + g.abs().sum(-1, keepdim=True) / D + xha * (g.abs() * xha).sum(-1, keepdim=True) / D)
            out["dx"] = (rs * (g - sg - xh * sgx), mag, 2 * nrow)
        if c.dwdb:
            n = -(-c.M // self.G) + self.G + 2
            dw, mdw, db, mdb = (dy * xh).sum(0), (dy.abs() * xha).sum(0), dy.sum(0), dy.abs().sum(0)
            if c.acc:
                dw, mdw = dw + inp["dw0"].to(dt), mdw + inp["dw0"].to(dt).abs()
                db, mdb = db + inp["db0"].to(dt), mdb + inp["db0"].to(dt).abs()
            out["dw"] = (dw, mdw, n + nrow)
            out["db"] = (db, mdb, n)
        return out

    def buffers(self, c, inp):
        b = {}
        if c.dx:
            b["dx"] = padded(c.M, c.D, BF16)
        if c.dwdb:
            b["dw"], b["db"] = padded(1, c.D, BF16, data=inp["dw0"]), padded(1, c.D, BF16, data=inp["db0"])
        return b

    def geom(self, c):
        return {"dx": dict(pass_cols=2048, row_stride=self.G), "dw": dict(row_stride=self.G), "db": dict(row_stride=self.G)}

    def drop_rows(self, c, inp, k):
        d = dict(inp)
        d["dy"] = inp["dy"].clone()
        d["dy"][c.M - k:] = 0
        return d

    def shift_pass(self, c, inp):
        if c.M <= self.G:
            return None
        d = dict(inp)
        hi = min(c.M - 1, 2 * self.G)
        for k in ("x", "dy"):
            d[k] = inp[k].clone()
            d[k][self.G:hi] = inp[k][self.G + 1:hi + 1]
        return d


class Colsum(Op):
    G = 64
    reduction_outs = ("out",)

    def __init__(self, f32):
        self.name = "colsum_f32" if f32 else "colsum"
        self.f32 = f32
        self.kinds = {"out": "f32" if f32 else "bf16"}
        shapes = [(R, 520, 528, 0) for R in (1, 63, 64, 65, 255, 256, 300)] + [(300, C, C, 0) for C in (8, 512)]
        shapes += [(300, 6, 8, 0), (300, 514, 516, 0), (300, 512, 512, 4)]       # the 2-column kernel: C % 8, ld % 8, a pointer 8 bytes off
        self.cases = [_case(f"R{R}-C{C}-ld{ld}-off{off}-acc{acc}", R=R, C=C, ld=ld, off=off, acc=acc)
                      for R, C, ld, off in shapes for acc in ((0,) if f32 else (0, 1))]

    def make(self, c):
        flat = torch.full((8 + c.R * c.ld + 8,), float("nan"), dtype=BF16)      # X = flat[8 + off:], [R][ld]; NaN past column C
        X = flat[8 + c.off:8 + c.off + c.R * c.ld]
        flat[8 + c.off:8 + c.off + (c.R - 1) * c.ld + c.C].unfold(0, c.C, c.ld)[:] = rnd(c.R, c.C, seed=3)
        return dict(flat=flat, X=X, out0=rnd(c.C, seed=5))

    def x(self, c, inp):
        return inp["flat"][8 + c.off:8 + c.off + (c.R - 1) * c.ld + c.C].unfold(0, c.C, c.ld)

    def formula(self, c, inp, dt):
        x = self.x(c, inp).to(dt)
        s, m = x.sum(0), x.abs().sum(0)
        if c.acc:
            s, m = s + inp["out0"].to(dt), m + inp["out0"].to(dt).abs()
        return {"out": (s, m, -(-c.R // self.G) + self.G + 2)}

    def buffers(self, c, inp):
        return {"out": padded(1, c.C, F32 if self.f32 else BF16, data=None if self.f32 else inp["out0"])}

    def geom(self, c):
        return {"out": dict(row_stride=self.G)}

    def drop_rows(self, c, inp, k):
        d = dict(inp)
        d["flat"] = inp["flat"].clone()
        self.x(c, d)[c.R - k:] = 0
        return d

    def shift_pass(self, c, inp):
        if c.R <= self.G + 1:
            return None
        d = dict(inp)
        d["flat"] = inp["flat"].clone()
        hi = min(c.R - 1, 2 * self.G)
        self.x(c, d)[self.G:hi] = self.x(c, inp)[self.G + 1:hi + 1]
        return d


def _sigmoid(g):
    return 1.0 / (1.0 + torch.exp(-g))


class Swiglu(Op):
    elementwise = True

    def __init__(self, bwd):
        self.name = "swiglu_bwd" if bwd else "swiglu_fwd"
        self.bwd = bwd
        self.kinds = {"gu": "bf16"} if bwd else {"act": "bf16"}
        self.cases = [_case(f"M{M}-I{I}", M=M, I=I) for M, I in ((123, 8), (1100, 7688))]

    def make(self, c):
        return dict(gu=rnd(c.M, 2 * c.I, seed=1, scale=2.0), dact=rnd(c.M, c.I, seed=2))

    def formula(self, c, inp, dt):
        g, u = inp["gu"][:, :c.I].to(dt), inp["gu"][:, c.I:].to(dt)
        sg = _sigmoid(g)
        if not self.bwd:
            o = g * sg * u
            return {"act": (o, torch.maximum(o.abs(), (g * sg).abs()), 4)}
        d = inp["dact"].to(dt)
        du = d * g * sg
        dg = d * u * sg * (1 + g * (1 - sg))
        mg = (d * u * sg).abs() * (1 + g.abs() * (1 + sg))      # 1 - sg: both of its terms count
        return {"gu": (torch.cat([dg, du], 1), torch.cat([mg, du.abs()], 1), 6)}

    def buffers(self, c, inp):
        return {"gu": padded(c.M, 2 * c.I, BF16, data=inp["gu"])} if self.bwd else {"act": padded(c.M, c.I, BF16)}

    def geom(self, c):
        return {} if self.bwd else {"act": dict(seam=8 * SEAM)}

    def seam_mask(self, c, name, b):
        """chunk i = 8 columns of act (forward), of dgate and of dup (backward), in row i / (I / 8)"""
        if not self.bwd:
            return Op.seam_mask(self, c, name, b)
        if c.M * (c.I // 8) <= SEAM:
            return None
        m = torch.zeros(c.M * c.I, dtype=torch.bool)
        m[8 * SEAM:] = True
        m = m.view(c.M, c.I)
        return torch.cat([m, m], 1)


class Gelu(Op):
    elementwise = True

    def __init__(self, bwd):
        self.name = "gelu_bwd" if bwd else "gelu_fwd"
        self.bwd = bwd
        self.kinds = {"dz": "bf16"} if bwd else {"h": "bf16"}
        self.cases = [_case(f"n{n}", n=n) for n in (8, 8 * (SEAM + 261))]

    def make(self, c):
        return dict(z=rnd(c.n, seed=3, scale=1.5), dh=rnd(c.n, seed=4))

    def formula(self, c, inp, dt):
        v = inp["z"].to(dt)
        e = torch.erf(v * 0.70710678118654752)
        if not self.bwd:
            return {"h": (0.5 * v * (1 + e), 0.5 * v.abs() * (1 + e.abs()), 4)}
        d = inp["dh"].to(dt)
        pdf = 0.3989422804014327 * torch.exp(-0.5 * v * v)
        return {"dz": (d * (0.5 * (1 + e) + v * pdf), d.abs() * (0.5 * (1 + e.abs()) + v.abs() * pdf * (1 + 0.5 * v * v)), 6)}

    def buffers(self, c, inp):
        return {"dz" if self.bwd else "h": padded(1, c.n, BF16)}

    def geom(self, c):
        return {"dz" if self.bwd else "h": dict(seam=8 * SEAM)}


def dropout_scale(p, alpha):
    return float(np.float32(alpha) / (np.float32(1.0) - np.float32(p)))          # the launcher's fp32 alpha / (1.f - p)


class Dropout(Op):
    name = "dropout"
    kinds = {"out": "bf16"}
    elementwise = True

    def __init__(self):
        self.cases = [_case(f"n{n}-add{add}", n=n, add=add, p=0.25, alpha=2.0, seed=1234567 + add) for n in (8, 8 * (SEAM + 261)) for add in (0, 1)]

    def make(self, c):
        return dict(x=rnd(c.n, seed=5), out0=rnd(c.n, seed=6), keep=O.dropout_mask(c.seed, c.n, c.p).bool())

    def formula(self, c, inp, dt):
        x = inp["x"].to(dt)
        sc = torch.tensor(dropout_scale(c.p, c.alpha), dtype=F64).to(dt)
        v = torch.where(inp["keep"], x * sc, torch.zeros_like(x))
        if c.add:
            o = inp["out0"].to(dt)
            return {"out": (o + v, o.abs() + v.abs(), 4)}
        return {"out": (v, v.abs(), 4)}

    def buffers(self, c, inp):
        return {"out": padded(1, c.n, BF16, data=inp["out0"] if c.add else None)}

    def geom(self, c):
        return {"out": dict(seam=8 * SEAM)}


class DropoutMask(Op):
    name = "dropout_mask"
    kinds = {"mask": "exact"}

    def __init__(self):
        self.cases = [_case(f"n{n}", n=n, p=0.1, seed=99) for n in (8, 8 * (SEAM + 261))]

    def make(self, c):
        return {}

    def exact(self, c, inp):
        return {"mask": O.dropout_mask(c.seed, c.n, c.p)}

    def buffers(self, c, inp):
        return {"mask": padded(1, c.n, torch.uint8)}

    def geom(self, c):
        return {"mask": dict(seam=8 * SEAM)}


def pack_bits(mask_u8):
    """bit e of byte g = element 8 g + e"""
    return torch.from_numpy(np.packbits(mask_u8.numpy().astype(np.uint8), bitorder="little"))


class DropoutBits(Op):
    name = "dropout_bits"
    kinds = {"bits": "exact"}

    def __init__(self):
        self.cases = [_case(f"n{n}", n=n, p=0.1, seed=99) for n in (32, 32 * (SEAM + 5))]

    def make(self, c):
        return {}

    def exact(self, c, inp):
        return {"bits": pack_bits(O.dropout_mask(c.seed, c.n, c.p))}

    def buffers(self, c, inp):
        return {"bits": padded(1, c.n // 8, torch.uint8)}

    def geom(self, c):
        return {"bits": dict(seam=4 * SEAM)}


def im2col_ref(px, P, Kp):
    n, _, S, _ = px.shape
    g = S // P
    ref = px.reshape(n, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(n * g * g, 3 * P * P)
    return torch.cat([ref, torch.zeros(n * g * g, Kp - 3 * P * P)], 1).bfloat16()


class Im2col(Op):
    name = "im2col"
    kinds = {"out": "exact"}

    def __init__(self):
        self.cases = [_case("n4-S336-P14-Kp592", n=4, S=336, P=14, Kp=592)]

    def make(self, c):
        return dict(px=rnd(c.n, 3, c.S, c.S, seed=8, dtype=F32))

    def exact(self, c, inp):
        return {"out": im2col_ref(inp["px"], c.P, c.Kp)}

    def buffers(self, c, inp):
        return {"out": padded(c.n * (c.S // c.P) ** 2, c.Kp, BF16)}

    def geom(self, c):
        return {"out": dict(seam=SEAM)}


def cast_values(n, seed):
    """random normals, then (as far as n allows) the special values: +-0, +-inf, the largest finite fp32, NaN, exact ties between two
    bf16 neighbours of both parities (subnormals are left out)"""
    x = rnd(n, seed=seed, dtype=F32) * 3
    ties = torch.tensor([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x7F7F8000, 0x00808000, 0x41FE8000, 0x41FF8000], dtype=torch.int64)
    sp = torch.cat([torch.tensor([0.0, -0.0, math.inf, -math.inf, 3.4028234663852886e38, -3.4028234663852886e38, math.nan]),
                    ties.to(torch.int32).view(F32)])
    k = min(n, sp.numel())
    x[n - k:] = sp[:k]
    return x


class Cast(Op):
    def __init__(self, to_bf16):
        self.name = "cast_f32_to_bf16" if to_bf16 else "cast_bf16_to_f32"
        self.to_bf16 = to_bf16
        self.kinds = {"dst": "exact"}
        self.cases = [_case(f"n{n}", n=n) for n in (1, 7, SEAM + 77)]

    def make(self, c):
        x = cast_values(max(c.n, 16), seed=c.n)[-c.n:] if c.n >= 7 else torch.tensor([1.00390625])      # n = 1: a tie (1 + 2^-8)
        return dict(src=x if self.to_bf16 else x.bfloat16())

    def exact(self, c, inp):
        return {"dst": inp["src"].bfloat16() if self.to_bf16 else inp["src"].float()}

    def buffers(self, c, inp):
        return {"dst": padded(1, c.n, BF16 if self.to_bf16 else F32)}

    def geom(self, c):
        return {"dst": dict(seam=SEAM)}


def shuffled(n, seed, mod=None):
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(n, generator=g).to(torch.int32) if mod is None else torch.randint(0, mod, (n,), generator=g).to(torch.int32)


class GatherRows(Op):
    name = "gather_rows"
    kinds = {"dst": "exact"}

    def __init__(self):
        self.cases = [_case(f"H{H}", H=H, N=9, R=7) for H in (8, 2048, 8192, 8200, 12288, 16392)]

    def make(self, c):
        return dict(src=rnd(c.N, c.H, seed=1), rows=torch.tensor([5, 0, 8, 5, 3, 8, 1], dtype=torch.int32))      # repeated, unsorted

    def exact(self, c, inp):
        return {"dst": inp["src"][inp["rows"].long()]}

    def buffers(self, c, inp):
        return {"dst": padded(c.R, c.H, BF16)}

    def geom(self, c):
        return {"dst": dict(pass_cols=2048)}


class ScatterRows(Op):
    name = "scatter_rows"
    kinds = {"dst": "exact"}

    def __init__(self):
        self.cases = [_case(f"H{H}", H=H, N=9, R=4) for H in (8, 2056)]

    def make(self, c):
        return dict(src=rnd(c.R, c.H, seed=1), rows=torch.tensor([7, 2, 8, 0], dtype=torch.int32), dst0=rnd(c.N, c.H, seed=2))

    def exact(self, c, inp):
        d = inp["dst0"].clone()
        d[inp["rows"].long()] = inp["src"]
        return {"dst": d}

    def buffers(self, c, inp):
        return {"dst": padded(c.N, c.H, BF16, data=inp["dst0"])}

    def geom(self, c):
        return {"dst": dict(pass_cols=2048)}


class RowsGather(Op):
    name = "rows_gather"
    kinds = {"dst": "exact"}

    def __init__(self):
        self.cases = [_case(f"W{W}", W=W, lds=W + 24, N=9, R=5) for W in (8, 2048, 2056)]

    def make(self, c):
        src = torch.full((c.N, c.lds), float("nan"), dtype=BF16)
        src[:, :c.W] = rnd(c.N, c.W, seed=1)
        return dict(src=src, rows=torch.tensor([6, 1, 8, 0, 3], dtype=torch.int32))

    def exact(self, c, inp):
        return {"dst": inp["src"][inp["rows"].long()][:, :c.W]}

    def buffers(self, c, inp):
        return {"dst": padded(c.R, c.W, BF16)}

    def geom(self, c):
        return {"dst": dict(pass_cols=2048)}


class RowsAdd(Op):
    name = "rows_add"
    kinds = {"dst": "exact"}

    def __init__(self):
        self.cases = [_case(f"W{W}", W=W, ldd=W + 24, N=9, R=5) for W in (8, 2048, 2056)]

    def make(self, c):
        return dict(src=rnd(c.R, c.W, seed=1), rows=torch.tensor([6, 1, 8, 0, 3], dtype=torch.int32), dst0=rnd(c.N, c.ldd, seed=2))

    def exact(self, c, inp):
        # the logical result is the WHOLE [N][ldd] matrix: untouched rows and the columns past W stay bit-identical
        d = inp["dst0"].clone()
        r = inp["rows"].long()
        d[r, :c.W] = (inp["src"].float() + inp["dst0"][r, :c.W].float()).bfloat16()
        return {"dst": d}

    def buffers(self, c, inp):
        return {"dst": padded(c.N, c.ldd, BF16, data=inp["dst0"])}

    def geom(self, c):
        return {"dst": dict(pass_cols=2048, width=c.W)}


class Rowdot(Op):
    name = "rowdot"
    kinds = {"out": "f32"}

    def __init__(self):
        self.cases = [_case(f"H{H}", M=5, H=H) for H in (8, 2048, 2056, 4104)]

    def make(self, c):
        return dict(X=rnd(c.M, c.H, seed=1), v=rnd(c.H, seed=2, dtype=F32))

    def formula(self, c, inp, dt):
        X, v = inp["X"].to(dt), inp["v"].to(dt)
        return {"out": ((X * v).sum(-1), (X * v).abs().sum(-1), n_acc(c.H) + 1)}

    def buffers(self, c, inp):
        return {"out": padded(1, c.M, F32)}

    reduction_outs = ("out",)

    def drop_rows(self, c, inp, k):
        """the last 8 k columns (one thread's chunk of the last pass) are missing from the dot product"""
        d = dict(inp)
        d["v"] = inp["v"].clone()
        d["v"][c.H - 8 * k:] = 0
        return d


def rope_tables_f32(max_pos, hd, theta=10000.0):
    """the cos / sin tables the kernel is GIVEN (an input of vlr_rope_heads; vlr_rope_table is not under test here)"""
    half = hd // 2
    inv = 1.0 / theta ** (torch.arange(half, dtype=F64) * 2 / hd)
    a = torch.arange(max_pos, dtype=F64)[:, None] * inv[None]
    return torch.cos(a).float(), torch.sin(a).float()


class RopeHeads(Op):
    name = "rope_heads"
    kinds = {"qkv": "bf16"}
    elementwise = True

    def __init__(self):
        self.cases = [_case(f"hd{hd}-bwd{bwd}", hd=hd, nh=5, ld=7 * hd + 8, M=53, max_pos=40, bwd=bwd) for hd in (16, 64, 128) for bwd in (0, 1)]

    def make(self, c):
        g = torch.Generator().manual_seed(4)
        pos = torch.randint(0, c.max_pos, (c.M,), generator=g).to(torch.int32)
        pos[3], pos[17], pos[52] = -3, c.max_pos + 2, c.max_pos - 1                # clamped by the kernel to [0, max_pos - 1]
        cos, sin = rope_tables_f32(c.max_pos, c.hd)
        return dict(qkv=rnd(c.M, c.ld, seed=1), pos=pos, cos=cos, sin=sin)

    def formula(self, c, inp, dt, x=None, bwd=None):
        x = (inp["qkv"] if x is None else x).to(dt)
        bwd = c.bwd if bwd is None else bwd
        p = inp["pos"].long().clamp(0, c.max_pos - 1)
        half = c.hd // 2
        cs, sn = inp["cos"][p].to(dt)[:, None, :], inp["sin"][p].to(dt)[:, None, :] * (-1.0 if bwd else 1.0)
        h = x[:, :c.nh * c.hd].reshape(c.M, c.nh, c.hd)
        x1, x2 = h[..., :half], h[..., half:]
        o = torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1).reshape(c.M, c.nh * c.hd)
        m = torch.cat([(x1 * cs).abs() + (x2 * sn).abs(), (x2 * cs).abs() + (x1 * sn).abs()], -1).reshape(c.M, c.nh * c.hd)
        return {"qkv": (o, m, 4)}

    def buffers(self, c, inp):
        W = c.nh * c.hd
        b = padded(c.M, W, BF16, ld=c.ld, data=inp["qkv"][:, :W])
        b.flat[b.off:b.off + c.M * c.ld].view(c.M, c.ld)[:, W:] = inp["qkv"][:, W:]      # real data beside the rotated heads: must stay bit-identical
        return {"qkv": b}


def build_rows_ref(labels, shared, pad=-100):
    Bn, S = labels.shape
    keep = labels[:, 1:] != pad
    if shared is not None:
        keep = keep & (shared != 0)
    idx = torch.nonzero(torch.nn.functional.pad(keep, (0, 1)).reshape(-1)).squeeze(1)
    tgt = labels.reshape(-1)[idx + 1]
    seq_off = torch.cat([torch.zeros(1, dtype=torch.long), keep.sum(-1).cumsum(0)])
    return idx.to(torch.int32), tgt.to(torch.int32), seq_off.to(torch.int32)


class BuildRows(Op):
    name = "build_rows"
    kinds = {"rows": "exact", "tgt": "exact", "seq_off": "exact"}

    def __init__(self):
        self.cases = [_case(f"S{S}-Bn{Bn}-shared{sh}", S=S, Bn=Bn, shared=sh) for S in (2, 1024, 1025, 1026, 2050) for Bn in (1, 3) for sh in (0, 1)]

    def make(self, c):
        g = torch.Generator().manual_seed(c.S + c.Bn)
        lab = torch.randint(0, 500, (c.Bn, c.S), generator=g)
        # one sequence kept only at positions 1022, 1023, 1024, 2047 (as far as S allows); with three: one all pad, one all kept
        lab[0] = -100
        for p in (1022, 1023, 1024, 2047):
            if p < c.S:
                lab[0, p] = 7 + p
        if c.S == 2:
            lab[0, 1] = 9
        if c.Bn == 3:
            lab[1] = -100
            lab[2] = torch.randint(0, 500, (c.S,), generator=g)
        shared = (torch.rand(c.Bn, c.S - 1, generator=g) < 0.7).to(torch.uint8) if c.shared else None
        if shared is not None:
            shared[0] = 1
        return dict(labels=lab, shared=shared)

    def exact(self, c, inp):
        rows, tgt, seq_off = build_rows_ref(inp["labels"], inp["shared"])
        return {"rows": rows, "tgt": tgt, "seq_off": seq_off}

    def buffers(self, c, inp):
        R = int(self.exact(c, inp)["seq_off"][-1])
        # the kernel writes R entries; the buffers are the caller's Bn * S: everything past R must keep its poison
        return {"rows": padded(1, max(R, 0), torch.int32, ld=c.Bn * c.S), "tgt": padded(1, max(R, 0), torch.int32, ld=c.Bn * c.S),
                "seq_off": padded(1, c.Bn + 1, torch.int32)}


def _logits(c):
    """fp32 [R][ld] with NaN past V; three score profiles over the rows"""
    g = torch.Generator().manual_seed(c.V)
    lg = torch.full((c.R, c.ld), float("nan"), dtype=F32)
    x = torch.randn(c.R, c.V, generator=g) * 3
    x[1] = torch.linspace(-30, 30, c.V) + 0.01 * torch.randn(c.V, generator=g)      # rising to the last column: every step rescales
    x[2] = -80.0
    x[2, (c.V * 2) // 3] = 80.0                                                     # one +80 spike among -80
    x[4] = torch.linspace(-20, 20, c.V)
    lg[:, :c.V] = x
    return lg


class LogpRows(Op):
    name = "logp_rows"
    kinds = {"lse": "f32", "tok": "f32"}
    reduction_outs = ("lse", "tok")

    def __init__(self):
        self.cases = [_case(f"V{V}-idx{idx}", V=V, ld=V + 4, R=5, idx=idx) for V in (4, 1020, 1024, 1028, 32064, 151936) for idx in (0, 1)]

    def make(self, c):
        tgt = torch.tensor([0, c.V - 1, (c.V * 2) // 3, c.V // 2, c.V - 1], dtype=torch.int32)
        return dict(logits=_logits(c), tgt=tgt, row_idx=torch.tensor([3, 0, 4, 2, 1], dtype=torch.int32) if c.idx else None)

    def rows(self, c, inp):
        l = inp["logits"][:, :c.V]
        return l[inp["row_idx"].long()] if c.idx else l

    def formula(self, c, inp, dt):
        l = self.rows(c, inp).to(dt)
        m = l.max(-1).values
        s = torch.exp(l - m[:, None]).sum(-1)
        z = m + torch.log(s)
        pick = l.gather(1, inp["tgt"].long()[:, None]).squeeze(1)
        n = 4 * -(-c.V // 1024) + 16 + 8
        mz = m.abs() + 1 + torch.log(s).abs()
        return {"lse": (z, mz, n), "tok": (pick - z, mz + pick.abs(), n + 1)}

    def emulate(self, c, inp):
        """the kernel's order: thread t takes columns 4 t + 1024 k, online max / sum (rescaled when its maximum moves), then the block
        maximum, the partial sums rescaled to it and summed"""
        l = self.rows(c, inp).float()
        steps = -(-c.V // 1024)
        lp = torch.full((c.R, steps * 1024), -math.inf)
        lp[:, :c.V] = l
        lp = lp.reshape(c.R, steps, 256, 4)
        m = torch.full((c.R, 256), -math.inf)
        s = torch.zeros(c.R, 256)
        for k in range(steps):
            v = lp[:, k]
            live = torch.isfinite(v[..., 0])
            mx = v.max(-1).values
            up = live & (mx > m)
            s = torch.where(up, s * torch.exp(torch.where(up, m - mx, torch.zeros_like(m))), s)
            m = torch.where(up, mx, m)
            s = torch.where(live, s + torch.exp(v - torch.where(live, m, torch.zeros_like(m))[..., None]).sum(-1), s)
        M = m.max(-1).values
        s = torch.where(torch.isinf(m), torch.zeros_like(s), s * torch.exp(torch.where(torch.isinf(m), torch.zeros_like(m), m - M[:, None])))
        z = M + torch.log(s.sum(-1))
        return {"lse": z, "tok": l.gather(1, inp["tgt"].long()[:, None]).squeeze(1) - z}

    def buffers(self, c, inp):
        return {"lse": padded(1, c.R, F32), "tok": padded(1, c.R, F32)}

    def drop_rows(self, c, inp, k):
        """the last 4 k columns (one thread's last load) are missing from the sum"""
        d = dict(inp)
        d["logits"] = inp["logits"].clone()
        d["logits"][:, c.V - 4 * k:c.V] = -math.inf
        return d


class DlogitsRows(Op):
    name = "dlogits_rows"
    kinds = {"dl": "bf16"}
    elementwise = True
    LENS = (3, 0, 1, 4)

    def __init__(self):
        self.cases = [_case(f"V{V}-avg{a}", V=V, ld=V + 4, ldd=V + 8, R=8, avg=a) for V in (8, 2048, 2056) for a in (0, 1)]

    def make(self, c):
        lg = torch.full((c.R, c.ld), float("nan"), dtype=F32)
        lg[:, :c.V] = rnd(c.R, c.V, seed=c.V, dtype=F32) * 3
        tgt = torch.tensor([0, 2047, 2048, 5, 0, 2047, 2048, 3], dtype=torch.int32).clamp(max=c.V - 1)
        lse = torch.logsumexp(lg[:, :c.V].double(), -1).float()                      # an input of the backward: the forward's fp32 lse
        seq_off = torch.tensor([0] + list(np.cumsum(self.LENS)), dtype=torch.int32)
        return dict(logits=lg, tgt=tgt, lse=lse, seq_off=seq_off, dlogps=rnd(len(self.LENS), seed=7, dtype=F32))

    def formula(self, c, inp, dt):
        l, z = inp["logits"][:, :c.V].to(dt), inp["lse"].to(dt)[:, None]
        lens = torch.tensor(self.LENS)
        seq = torch.repeat_interleave(torch.arange(len(self.LENS)), lens)
        g = inp["dlogps"].to(dt)[seq]
        if c.avg:
            g = g / lens[seq].to(dt)
        p = torch.exp(l - z)
        one = torch.nn.functional.one_hot(inp["tgt"].long(), c.V).to(dt)
        return {"dl": (g[:, None] * (one - p), g.abs()[:, None] * (one + p * (1 + l.abs() + z.abs())), 6)}

    def buffers(self, c, inp):
        return {"dl": padded(c.R, c.V, BF16, ld=c.ldd)}

    def geom(self, c):
        return {"dl": dict(pass_cols=2048)}


class SeqSum(Op):
    name = "seq_sum"
    kinds = {"out": "f32"}
    reduction_outs = ("out",)

    def __init__(self):
        self.cases = [_case("lens-avg0", lens=(1, 255, 256, 257, 1000), avg=0), _case("lens-avg1", lens=(1, 255, 256, 257, 1000), avg=1),
                      _case("zero-length-avg0", lens=(1, 0, 255, 256, 0, 257, 1000), avg=0)]

    def make(self, c):
        return dict(tok=-rnd(sum(c.lens), seed=3, dtype=F32).abs() * 4, seq_off=torch.tensor([0] + list(np.cumsum(c.lens)), dtype=torch.int32))

    def formula(self, c, inp, dt):
        t = inp["tok"].to(dt)
        o, m = [], []
        for lo, hi in zip(inp["seq_off"][:-1].tolist(), inp["seq_off"][1:].tolist()):
            s, a = t[lo:hi].sum(), t[lo:hi].abs().sum()
            if c.avg:
                s, a = s / (hi - lo), a / (hi - lo)
            o.append(s)
            m.append(a)
        return {"out": (torch.stack(o), torch.stack(m), n_acc(max(c.lens)) + 1)}

    def buffers(self, c, inp):
        return {"out": padded(1, len(c.lens), F32)}

    def drop_rows(self, c, inp, k):
        d = dict(inp)
        d["tok"] = inp["tok"].clone()
        d["tok"][-k:] = 0
        return d


LOSS_IDS = {"sigmoid": 0, "ddpo": 0, "hinge": 1, "ipo": 2, "kto_pair": 3}


class DpoLoss(Op):
    name = "dpo_loss"
    kinds = {k: "f32" for k in ("losses", "cr", "rr", "dpc", "dpr", "mean")}
    reduction_outs = ("mean",)
    BETA = 0.3

    def __init__(self):
        self.cases = []
        for n in (1, 63, 64, 65, 1000, 1024):
            for lt in LOSS_IDS:
                grid = [(ls, rf, up) for ls in (0.0, 0.2) for rf in (0, 1) for up in (0, 1)] if n in (65, 1024) else [(0.0, 0, 0), (0.2, 1, 1)]
                signs = ((1, 1), (1, -1), (-1, 1), (-1, -1)) if lt == "kto_pair" else ((1, 1),)
                for ls, rf, up in grid:
                    for sc, sr in (signs if (ls, rf, up) == grid[0] else signs[:1]):
                        self.cases.append(_case(f"n{n}-{lt}-ls{ls}-rf{rf}-up{up}-kl{sc:+d}{sr:+d}", n=n, lt=lt, ls=ls, rf=rf, up=up, sc=sc, sr=sr))

    def make(self, c):
        g = torch.Generator().manual_seed(7 + c.n)
        n = c.n
        rc, rr = torch.randn(n, generator=g) * 4 - 30, torch.randn(n, generator=g) * 4 - 30
        # beta (pc - pr) sweeps [-100, 100] (n = 1: -100): the log-sigmoid / sigmoid tails; kto: the two clamped means take both signs
        sweep = torch.linspace(-100.0, 100.0, n) / self.BETA if n > 1 else torch.tensor([-100.0 / self.BETA])
        sweep = sweep[torch.randperm(n, generator=g)]
        pc = rc + 3.0 * c.sc + torch.randn(n, generator=g) + sweep / 2
        pr = rr + 3.0 * c.sr + torch.randn(n, generator=g) - sweep / 2
        nl = 2 * n if c.lt == "kto_pair" else n
        return dict(pc=pc, pr=pr, rc=rc, rr=rr, up=torch.randn(nl, generator=g) if c.up else None)

    def formula(self, c, inp, dt):
        pc, pr = inp["pc"].to(dt).requires_grad_(True), inp["pr"].to(dt).requires_grad_(True)
        losses, cr, rr = O.dpo_loss(pc, pr, inp["rc"].to(dt), inp["rr"].to(dt), float(np.float32(self.BETA)), float(np.float32(c.ls)),
                                    c.lt, bool(c.rf))      # beta, label_smoothing: the launcher's fp32 arguments
        if inp["up"] is not None:
            (losses * inp["up"].to(dt)).sum().backward()
        else:
            losses.mean().backward()
        # the tolerances of tests/test_hip_kernels.py::test_dpo_loss_fwd_bwd, as (rtol, atol), elementwise
        ga = 2e-6 if inp["up"] is not None else 2e-7
        return {"losses": (losses.detach(), None, (2e-5, 2e-6)), "cr": (cr.detach(), None, (1e-5, 1e-6)), "rr": (rr.detach(), None, (1e-5, 1e-6)),
                "dpc": (pc.grad, None, (2e-4, ga)), "dpr": (pr.grad, None, (2e-4, ga)), "mean": (losses.detach().mean().reshape(1), None, (2e-5, 1e-6))}

    def buffers(self, c, inp):
        nl = 2 * c.n if c.lt == "kto_pair" else c.n
        b = {k: padded(1, c.n, F32) for k in ("cr", "rr", "dpc", "dpr")}
        b["losses"], b["mean"] = padded(1, nl, F32), padded(1, 1, F32)
        return b

    def drop_rows(self, c, inp, k):
        """the last pair is missing from the mean (and, kto_pair, from the two KL means)"""
        if c.n < 2:
            return None
        d = {kk: (v[:c.n - k] if v is not None and kk != "up" else v) for kk, v in inp.items()}
        if inp["up"] is not None:
            d["up"] = torch.cat([inp["up"][:c.n - k], inp["up"][c.n:2 * c.n - k]]) if c.lt == "kto_pair" else inp["up"][:c.n - k]
        return d


class GradSqnorm(Op):
    name = "grad_sqnorm"
    kinds = {"out3": "f32"}
    reduction_outs = ("out3",)
    BLOCKS = 1024

    def __init__(self):
        self.cases = [_case(f"n8_{n8}-gs{gs}-ex{ex}-mn{mn}", n8=n8, gscale=gs, extra=ex, max_norm=mn)
                      for n8 in (1, 769, 6 * 262144 + 300) for gs in (1.0, 0.125) for ex in (0.0, 2.5) for mn in (0.0, 1.0, 1e6)]

    def make(self, c):
        return dict(g=rnd(8 * c.n8, seed=1, scale=0.05))

    def _out3(self, c, s, dt):
        gs, ex, mn = (torch.tensor(v, dtype=F32).to(dt) for v in (c.gscale, c.extra, c.max_norm))
        nrm = torch.sqrt(s * gs * gs + ex)
        coef = (torch.minimum(torch.ones((), dtype=dt), mn / (nrm + torch.tensor(1e-6, dtype=F32).to(dt))) if c.max_norm > 0 else torch.ones((), dtype=dt)) * gs
        return torch.stack([nrm, coef, s])

    def formula(self, c, inp, dt):
        g = inp["g"].to(dt)
        o = self._out3(c, (g * g).sum(), dt)
        P = min(-(-c.n8 // 256), self.BLOCKS)
        n = 8 * -(-c.n8 // (P * 256)) + 10 + -(-P // 256) + 10 + 6
        return {"out3": (o, o.abs(), n)}

    def emulate(self, c, inp):
        """partials per workgroup (chunk i of 8 belongs to workgroup (i mod P 256) / 256), then their sum in one workgroup"""
        g = inp["g"].float().reshape(c.n8, 8)
        P = min(-(-c.n8 // 256), self.BLOCKS)
        sq = (g * g).sum(-1)
        k = -(-c.n8 // (P * 256))
        sq = torch.cat([sq, torch.zeros(k * P * 256 - c.n8)]).reshape(k, P, 256)
        part = sq.sum(0).sum(-1)
        return {"out3": self._out3(c, part.sum(), F32)}

    def buffers(self, c, inp):
        return {"out3": padded(1, 3, F32)}

    def drop_rows(self, c, inp, k):
        d = dict(inp)
        d["g"] = inp["g"].clone()
        d["g"][-8 * k:] = 0
        return d


class Adamw(Op):
    name = "adamw_step"
    kinds = {"master": "f32", "m": "f32", "v": "f32"}
    elementwise = True
    HP = dict(lr=1e-3, beta1=0.9, beta2=0.98, eps=1e-6)

    def __init__(self):
        self.cases = [_case(f"n8_{n8}-coef{cf}-step{st}-wd{wd}", n8=n8, coef=cf, step=st, wd=wd)
                      for n8 in (1, 524288 + 3 * 256 + 5) for cf in (0, 1) for st in (1, 2, 1000) for wd in (0.0, 0.05)]

    def make(self, c, coef=None):
        """coef: the out3[1] of a clipping vlr_grad_sqnorm over the same gradient (the GPU test passes the kernel's); default: its
        fp32 emulation"""
        n = 8 * c.n8
        if c.coef and coef is None:
            sq = OPS["grad_sqnorm"]
            cc = _case("clip", n8=c.n8, gscale=1.0, extra=0.0, max_norm=0.01)
            coef = float(sq.emulate(cc, dict(g=rnd(n, seed=4, scale=0.01)))["out3"][1])
        return dict(master=rnd(n, seed=1, dtype=F32), m=rnd(n, seed=2, scale=0.01, dtype=F32), v=rnd(n, seed=3, scale=0.01, dtype=F32) ** 2,
                    g=rnd(n, seed=4, scale=0.01), coef=coef)                      # coef: the out3[1] of a clipping grad_sqnorm (an input)

    def formula(self, c, inp, dt):
        f = lambda v: torch.tensor(v, dtype=F32).to(dt)                           # noqa: E731  (the launcher's fp32 arguments)
        hp = self.HP
        lr, b1, b2, eps, wd = f(hp["lr"]), f(hp["beta1"]), f(hp["beta2"]), f(hp["eps"]), f(c.wd)
        bc1 = f(float(np.float32(1) - np.float32(np.power(np.float32(hp["beta1"]), np.float32(c.step)))))
        bc2 = np.float32(1) - np.float32(np.power(np.float32(hp["beta2"]), np.float32(c.step)))
        rb = f(float(np.float32(1) / np.sqrt(bc2)))
        coef = f(float(inp["coef"])) if inp["coef"] is not None else f(1.0)
        w, m, v, g = inp["master"].to(dt), inp["m"].to(dt), inp["v"].to(dt), inp["g"].to(dt) * coef
        w1 = w * (1 - lr * wd)
        m1 = b1 * m + (1 - b1) * g
        v1 = b2 * v + (1 - b2) * g * g
        upd = (lr / bc1) * m1 / (torch.sqrt(v1) * rb + eps)
        mm = (b1 * m).abs() + ((1 - b1) * g).abs()
        return {"master": (w1 - upd, w1.abs() + 4 * (lr / bc1) * mm / (torch.sqrt(v1) * rb + eps), 6), "m": (m1, mm, 4), "v": (v1, v1, 6)}

    def buffers(self, c, inp):
        n = 8 * c.n8
        return {"master": padded(1, n, F32, data=inp["master"]), "m": padded(1, n, F32, data=inp["m"]), "v": padded(1, n, F32, data=inp["v"]),
                "p16": padded(1, n, BF16)}

    def geom(self, c):
        s = 8 * 2048 * 256
        return {k: dict(seam=s) for k in ("master", "m", "v")}


class MergeFwdF32(Op):
    """src comes from vlr_merge_index on the GPU (as tests/test_hip_kernels.py::test_merge_matches_oracle); on the CPU the same map is
    written down by hand: text token t, image feature row -(f + 1), SRC_ZERO"""
    name = "merge_fwd_f32"
    kinds = {"out": "exact"}
    SRC_ZERO = -(2 ** 31)

    def __init__(self):
        self.cases = [_case(f"H{H}-f32feats{f}", H=H, feats_f32=f, Bn=6, T=12, P=5, V=90) for H in (8, 2056) for f in (0, 1)]

    def make(self, c):
        g = torch.Generator().manual_seed(3)
        Bh, T, image_token = c.Bn // 2, c.T, 80
        ids_h = torch.randint(3, 80, (Bh, T), generator=g)
        ids_h[:, 0] = 1
        for b in range(Bh):
            ids_h[b, 2 + b] = image_token
        ids = torch.cat([ids_h, ids_h.clone()], 0)
        ids[Bh:, 8:] = torch.randint(3, 80, (Bh, T - 8), generator=g)
        am = torch.ones_like(ids)
        ids[1, 10:], am[1, 10:], ids[4, 9:], am[4, 9:] = 81, 0, 81, 0           # the model's pad token: zero rows in the output
        lab = ids.clone()
        lab[am == 0] = -100
        feats = rnd(Bh * c.P, c.H, seed=2, dtype=F32)
        return dict(ids=ids, am=am, lab=lab, table=rnd(c.V, c.H, seed=1), feats=feats if c.feats_f32 else feats.bfloat16(), image_token=image_token,
                    model_pad=81, S=T - 1 + c.P)

    def exact_from_src(self, c, inp, src):
        """src int32 [Bn][S] -> out fp32 [Bn * S][H]"""
        S = inp["S"]
        out = torch.zeros(c.Bn * S, c.H, dtype=F32)
        s = src.reshape(-1).long()
        b = torch.arange(c.Bn * S) // S
        text = s >= 0
        out[text] = inp["table"][inp["ids"][b[text], s[text]]].float()
        img = (s < 0) & (s != self.SRC_ZERO)
        out[img] = inp["feats"][-(s[img] + 1)].float()
        return out

    def cpu_src(self, c, inp):
        """every row holds one image and ends in a non-pad token: no shift; text token t lands on its running position, the free
        positions are the image slots in order, feature row = global slot rank mod the number of (deduplicated) feature rows"""
        S, n = inp["S"], inp["feats"].shape[0]
        src = torch.full((c.Bn, S), self.SRC_ZERO, dtype=torch.int64)
        k = 0
        for b in range(c.Bn):
            pos, taken = -1, set()
            for t in range(c.T):
                tok = int(inp["ids"][b, t])
                pos += c.P if tok == inp["image_token"] else 1
                if tok != inp["image_token"]:
                    taken.add(pos)
                    if tok != inp["model_pad"]:
                        src[b, pos] = t
            for s_ in range(S):
                if s_ not in taken:
                    src[b, s_] = -((k % n) + 1)
                    k += 1
        return src.to(torch.int32)

    def exact(self, c, inp):
        return {"out": self.exact_from_src(c, inp, inp["src"] if "src" in inp else self.cpu_src(c, inp))}

    def buffers(self, c, inp):
        return {"out": padded(c.Bn * inp["S"], c.H, F32)}

    def geom(self, c):
        return {"out": dict(pass_cols=2048)}


OPS = {o.name: o for o in (
    RmsnormFwd(False), RmsnormFwd(True), RmsnormBwd(False), RmsnormBwd(True), LayernormFwd(False), LayernormFwd(True), LayernormBwd(),
    Colsum(False), Colsum(True), Swiglu(False), Swiglu(True), Gelu(False), Gelu(True), Dropout(), DropoutMask(), DropoutBits(), Im2col(),
    Cast(True), Cast(False), GatherRows(), ScatterRows(), RowsGather(), RowsAdd(), Rowdot(), RopeHeads(), BuildRows(), LogpRows(),
    DlogitsRows(), SeqSum(), DpoLoss(), GradSqnorm(), Adamw(), MergeFwdF32())}


def all_cases(ops=None):
    return [(n, c) for n, o in OPS.items() if ops is None or n in ops for c in o.cases]


def case_id(p):
    return f"{p[0]}-{p[1].name}"


def place(op, c, inp, outs):
    """-> ({output: Buf}, {output: flat buffer with `outs` written into the logical result})"""
    op = OPS[op] if isinstance(op, str) else op
    bufs = op.buffers(c, inp)
    after = {}
    for k, b in bufs.items():
        if k not in outs:
            continue
        f = b.flat.clone()
        logical(b, f)[:] = outs[k].reshape(b.rows, b.width).to(f.dtype)
        after[k] = f
    return bufs, after


def measure_tol(ops=None):
    """worst |unrounded fp32 emulation - float64 reference| / mag per operation and output over its cases (how TOL was obtained)"""
    res = {}
    for name in (ops or TOL):
        op = OPS[name]
        for c in op.cases:
            inp = op.make(c)
            ref, emu = op.formula(c, inp, F64), op.emulate(c, inp)
            for k, (val, mag, _) in ref.items():
                e = float(((emu[k].to(F64) - val).abs() / mag.clamp_min(1e-300)).max())
                res.setdefault(name, {})[k] = max(res.get(name, {}).get(k, 0.0), e)
    return res


if __name__ == "__main__":
    for name, d in measure_tol().items():
        print(name, {k: (float(f"{v:.2g}"), float(f"{4 * v:.2g}")) for k, v in d.items()})
