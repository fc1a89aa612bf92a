"""The checkers of tests/row_ref.py, on the CPU: for every case of tests/test_hip_row_edges.py the fp32 emulation of the operation passes
its checker (the tolerances are reachable by a correct fp32 implementation on exactly these inputs), and each simulated kernel fault
fails the checker on every case it applies to."""
import functools

import pytest
import torch

from tests import row_ref as R

ALL = R.all_cases()


_SMALL = {}


@functools.lru_cache(maxsize=2)
def _prepared(name, cname):
    op = R.OPS[name]
    c = next(c for c in op.cases if c.name == cname)
    inp = op.make(c)
    return op, c, inp, R.expect(op, c, inp), R.emulate_fp32(op, c, inp)


def prepared(name, cname):
    """the case's inputs, expectation and emulation, computed once for both tests where they are small (under 1 M input elements)"""
    if (name, cname) not in _SMALL:
        r = _prepared(name, cname)
        if sum(v.numel() for v in r[2].values() if isinstance(v, torch.Tensor)) > 1 << 20:
            return r
        _SMALL[name, cname] = r
    return _SMALL[name, cname]


@pytest.mark.parametrize("p", ALL, ids=[R.case_id(p) for p in ALL])
def test_fp32_emulation_passes_its_checker(p):
    op, c, inp, exp, emu = prepared(p[0], p[1].name)
    bufs, after = R.place(op, c, inp, emu)
    assert set(after) == set(exp), (set(after), set(exp))
    for k in after:
        R.check(f"{op.name} {c.name} {k}", after[k], bufs[k], exp[k])


# ---------------------------------------------------------------------------------------------------- simulated faults
# each generator yields (output, faulty flat buffer) for every output of the case the fault applies to
def _written_width(op, c, k, b):
    return op.geom(c).get(k, {}).get("width", b.width)


def stale_last_pass(op, c, inp, exp, emu, bufs, after):
    """the columns of the last loop pass keep what the buffer held before the call"""
    for k, b in bufs.items():
        g = op.geom(c).get(k, {})
        if "pass_cols" not in g or k not in after:
            continue
        W = _written_width(op, c, k, b)
        start = (W - 1) // g["pass_cols"] * g["pass_cols"]
        f = after[k].clone()
        R.logical(b, f)[:, start:W] = R.logical(b)[:, start:W]
        yield k, f


def stale_from_seam(op, c, inp, exp, emu, bufs, after):
    """everything the second and later passes of the grid-stride loop write keeps what the buffer held before the call"""
    for k, b in bufs.items():
        m = op.seam_mask(c, k, b) if k in after else None
        if m is None:
            continue
        f = after[k].clone()
        lo = R.logical(b, f)
        lo[m] = R.logical(b)[m]
        yield k, f


def _emulated_with(op, c, inp, changed, bufs, after, only):
    outs = R.emulate_fp32(op, c, changed)
    for k in only:
        if k in after:
            f = after[k].clone()
            R.logical(bufs[k], f)[:] = outs[k].reshape(bufs[k].rows, bufs[k].width).to(f.dtype)
            yield k, f


def missing_rows(op, c, inp, exp, emu, bufs, after):
    """the last row (chunk, column group, pair), or the last partial block of rows, is missing from a reduction"""
    if op.name == "dpo_loss":                                   # the sum lacks the last pair, the divisor is unchanged
        n, l = c.n, emu["losses"].double()
        if n < 2:
            return
        tot = l.sum() - l[n - 1] - (l[2 * n - 1] if c.lt == "kto_pair" else 0.0)
        f = after["mean"].clone()
        R.logical(bufs["mean"], f)[:] = (tot / l.numel()).float()
        yield "mean", f
        return
    if not hasattr(op, "drop_rows"):
        return
    ks = {1}
    G = getattr(op, "G", None)
    M = c.get("M", c.get("R"))
    if G and M and M > G and M % G:
        ks.add(M % G)
    if op.name == "grad_sqnorm" and c.n8 > op.BLOCKS * 256:      # the chunks of the last, partial pass of the grid (the remainder loop's tail)
        ks.add(c.n8 % (op.BLOCKS * 256))
    for k in sorted(ks):
        changed = op.drop_rows(c, inp, k)
        if changed is not None:
            yield from _emulated_with(op, c, inp, changed, bufs, after, op.reduction_outs)


def second_pass_shifted(op, c, inp, exp, emu, bufs, after):
    """the second stride pass works on the data of the next row (row-strided kernels) / the next 8-element chunk (grid-stride loops)"""
    if hasattr(op, "shift_pass"):
        changed = op.shift_pass(c, inp)
        if changed is not None:
            yield from _emulated_with(op, c, inp, changed, bufs, after, list(after))
        return
    for k, b in bufs.items():
        seam = op.geom(c).get(k, {}).get("seam")
        n = b.rows * b.width
        if k not in after or seam is None or seam + 8 >= n or b.ld != b.width:
            continue
        f = after[k].clone()
        lo, src = R.logical(b, f).reshape(-1), R.logical(b, after[k]).reshape(-1)
        lo[seam:min(2 * seam, n) - 8] = src[seam + 8:min(2 * seam, n)]
        yield k, f


def two_ulp_tail(op, c, inp, exp, emu, bufs, after):
    """one element of the tail (the last 8 the kernel writes) is off by 2 bf16 ulps (an exact output: by one unit)"""
    for k, b in bufs.items():
        if k not in after or b.width == 0:
            continue
        W = _written_width(op, c, k, b)
        e = exp[k]
        ref = e.ref.reshape(b.rows, b.width).double()
        score = ref.abs() / (e.mag.reshape(b.rows, b.width) if e.rel is not None else 1.0)
        r = b.rows - 1
        if op.name == "rows_add":                               # the last row the kernel writes
            r = int(inp["rows"].max())
        lo_c = max(0, W - 8) if op.name != "dpo_loss" else 0    # dpo_loss: one thread per pair, no loop tail - the largest value
        j = lo_c + int(torch.nan_to_num(score[r, lo_c:W], nan=-1.0).argmax())
        f = after[k].clone()
        lo = R.logical(b, f)
        if lo.dtype == torch.bfloat16:
            R._bits(lo)[r, j] += 2
        elif lo.dtype == torch.float32:
            R._bits(lo)[r, j] += 2 << 16
        else:
            lo[r, j] ^= 1
        yield k, f


def poison_overwritten(op, c, inp, exp, emu, bufs, after):
    """one cell beside the result is written: the cell behind the last logical element, the cell in front of the first, and (strided
    results) the first padding column of the first row"""
    for k, b in bufs.items():
        if k not in after:
            continue
        cells = [b.off - 1, b.off + (b.rows - 1) * b.ld + b.width]
        if b.ld > b.width:
            cells.append(b.off + b.width)
        for i in cells:
            f = after[k].clone()
            f[i] = 0
            yield k, f


def _resolvable(f, good, b, e):
    """vlr_dpo_loss keeps the (rtol, atol) of tests/test_hip_kernels.py::test_dpo_loss_fwd_bwd: a saturated pair has a loss / gradient below
    atol, and dropping it from the mean or moving it by 2 bf16 ulps is under what those tolerances resolve.  The fault counts where it moves
    the output by more than twice the bound."""
    d = (R.logical(b, f).double() - R.logical(b, good).double()).abs()
    bound = e.rel * e.ref.reshape(b.rows, b.width).abs() + e.coef * e.mag.reshape(b.rows, b.width)
    return bool((d > 2 * bound).any())


FAULTS = [stale_last_pass, stale_from_seam, missing_rows, second_pass_shifted, two_ulp_tail, poison_overwritten]


@pytest.mark.parametrize("name", list(R.OPS))
def test_simulated_faults_fail_the_checker(name):
    op = R.OPS[name]
    applied = {f.__name__: 0 for f in FAULTS}
    missed = []
    for c in op.cases:
        _, _, inp, exp, emu = prepared(name, c.name)
        bufs, after = R.place(op, c, inp, emu)
        for fault in FAULTS:
            for k, f in fault(op, c, inp, exp, emu, bufs, after):
                if torch.equal(R._bits(f), R._bits(after[k])):
                    continue                                     # the fault changes nothing here (a stale cell that already held the result)
                if name == "dpo_loss" and fault in (missing_rows, two_ulp_tail) and not _resolvable(f, after[k], bufs[k], exp[k]):
                    continue
                if name == "grad_sqnorm" and fault is missing_rows and not _resolvable(f, after[k], bufs[k], exp[k]):
                    continue                                     # one chunk of 8 among 1.5 M: below what an fp32 sum of that length resolves
                applied[fault.__name__] += 1
                try:
                    R.check(f"{name} {c.name} {k}", f, bufs[k], exp[k])
                except AssertionError:
                    continue
                missed.append(f"{fault.__name__} on {c.name} {k}")
    assert not missed, f"{name}: the checker passed " + ", ".join(missed[:20])
    assert applied["two_ulp_tail"] and applied["poison_overwritten"], applied
    for f in ("stale_last_pass", "stale_from_seam", "missing_rows", "second_pass_shifted"):
        assert applied[f] or f not in EXPECTED.get(name, ()), (name, f, applied)


# which structural faults must find at least one case in an operation's table (the loops its launcher has)
_ROW = ("stale_last_pass",)
_SEAM = ("stale_from_seam", "second_pass_shifted")
EXPECTED = {
    "rmsnorm_fwd": _ROW, "rmsnorm_fwd_f32": _ROW, "layernorm_fwd": _ROW, "vit_embed_ln": _ROW,
    "rmsnorm_bwd": _ROW + ("missing_rows", "second_pass_shifted"), "rmsnorm_bwd_f32": _ROW + ("missing_rows", "second_pass_shifted"),
    "layernorm_bwd": _ROW + ("missing_rows", "second_pass_shifted"),
    "colsum": ("missing_rows", "second_pass_shifted"), "colsum_f32": ("missing_rows", "second_pass_shifted"),
    "swiglu_fwd": _SEAM, "swiglu_bwd": ("stale_from_seam",), "gelu_fwd": _SEAM, "gelu_bwd": _SEAM, "dropout": _SEAM, "dropout_mask": _SEAM,
    "dropout_bits": _SEAM, "im2col": _SEAM, "cast_f32_to_bf16": _SEAM, "cast_bf16_to_f32": _SEAM, "adamw_step": _SEAM,
    "gather_rows": _ROW, "scatter_rows": _ROW, "rows_gather": _ROW, "rows_add": _ROW, "merge_fwd_f32": _ROW, "dlogits_rows": _ROW,
    "rowdot": ("missing_rows",), "logp_rows": ("missing_rows",), "seq_sum": ("missing_rows",), "dpo_loss": ("missing_rows",),
    "grad_sqnorm": ("missing_rows",),
}


def test_every_operation_is_listed():
    assert set(EXPECTED) | {"rope_heads", "build_rows"} == set(R.OPS)


def test_checker_messages_and_poison():
    b = R.padded(2, 8, torch.bfloat16, ld=16)
    ref = torch.ones(2, 8, dtype=torch.float64)
    e = R.Exp(ref, ref, R.U_BF16, 4 * R.U_F32)
    good = b.flat.clone()
    R.logical(b, good)[:] = 1.0
    R.check("ok", good, b, e)
    bad = good.clone()
    R.logical(b, bad)[1, 3] = 1.0078125                          # one bf16 ulp above 1: 2^-7 > 2^-8
    with pytest.raises(AssertionError, match=r"\[1\]\[3\]"):
        R.check("x", bad, b, e)
    bad = good.clone()
    R.logical(b, bad)[0, 7] = float("nan")                       # an unwritten cell
    with pytest.raises(AssertionError, match=r"\[0\]\[7\]"):
        R.check("x", bad, b, e)
    bad = good.clone()
    bad[b.off + 8] = 1.0                                         # the padding column behind row 0
    with pytest.raises(AssertionError, match="overwritten"):
        R.check("x", bad, b, e)
    # exact outputs: -0 is not +0, NaN stays NaN
    b = R.padded(1, 3, torch.float32)
    ref = torch.tensor([0.0, float("nan"), 1.0])
    good = b.flat.clone()
    R.logical(b, good)[:] = ref
    R.check("ok", good, b, R.Exp(ref, None, None, None))
    bad = good.clone()
    R.logical(b, bad)[0, 0] = -0.0
    with pytest.raises(AssertionError, match="exactly"):
        R.check("x", bad, b, R.Exp(ref, None, None, None))
    bad = good.clone()
    R.logical(b, bad)[0, 1] = 5.0
    with pytest.raises(AssertionError, match="exactly"):
        R.check("x", bad, b, R.Exp(ref, None, None, None))
