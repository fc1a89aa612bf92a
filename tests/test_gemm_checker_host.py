"""The checker of tests/gemm_ref.py, on the CPU: for every case of tests/test_hip_gemm_edges.py the fp32 emulation of the GEMM passes the
checker (bitwise in the exact regime: the bound and the data are reachable by a correct fp32 implementation on exactly these inputs; large
cases on a row-and-column sample that holds every tile edge), the case table meets every entry point's alignment rules (the GPU file
never skips), and each planted fault is rejected."""
import functools

import pytest
import torch

from tests import gemm_ref as G

IDS = [c.name for c in G.CASES]


@functools.lru_cache(maxsize=4)
def prepared(name):
    c = G.BY_NAME[name]
    inp = G.make(c)
    rows, cols = G.sample(c)
    return c, inp, rows, cols, G.expect(c, inp, "cpu", rows, cols)


@pytest.mark.parametrize("name", IDS)
def test_fp32_emulation_passes_its_checker(name):
    c, inp, rows, cols, exp = prepared(name)
    b, after = G.place(c, inp, G.emulate(c, inp, rows, cols), rows, cols)
    G.check(name, after, b, exp)


@pytest.mark.parametrize("name", IDS)
def test_case_table_is_aligned_and_padded(name):
    c = G.BY_NAME[name]
    assert not G.alignment_errors(c), G.alignment_errors(c)
    a_w = c.M if c.layout == 2 else c.K
    b_w = c.K if c.layout == 0 else c.N
    # a read or a write into the padding is visible (vlr_gemm_lora takes W without a leading dimension: its guards remain)
    assert c.lda > a_w and (c.ldb > b_w or c.K2) and c.ldc > c.groups * c.N and c.ldr > c.N and (not c.K2 or c.ldu > c.K2)
    assert c.regime == "gauss" or c.act == 0
    assert isinstance(c.uses_256p, bool) and isinstance(c.split_k, bool) and c.split_k == bool(c.splits)


def test_coverage_rules():
    """every route: exact cases in the layouts that reach it, the epilogue set, a gauss case; act 1 and act 2 wherever an epilogue can run"""
    by = {}
    for c in G.CASES:
        by.setdefault(c.group, []).append(c)
    assert set(by) == {"ring", "staged", "tnsplit", "skinny", "gensplit", "tile256", "pers256", "cont", "peel", "grouped", "lora", "pair"}
    for g in ("grouped", "lora", "pair"):              # entry points of their own: one epilogue each (checked below the loop)
        by.pop(g)
    lays = {"ring": {0, 1, 2}, "staged": {1, 2}, "tnsplit": {2}, "skinny": {0, 1}, "gensplit": {0, 1}, "tile256": {0, 1, 2},
            "pers256": {0, 1, 2}, "cont": {0, 1, 2}, "peel": {0, 1}}
    for g, cs in by.items():
        assert {c.layout for c in cs if c.regime == "exact"} == lays[g], g
        assert any(c.res == "f32" and c.inplace for c in cs) or g == "staged", g
        if g not in ("peel",):
            assert any(c.regime == "gauss" for c in cs), g
        if g not in ("cont", "staged", "peel"):
            assert {c.act for c in cs} == {0, 1, 2}, g
            assert any(c.bias and c.res == "bf16" and c.acc and c.alpha == 0.5 and c.ldc >= c.N + 1000 for c in cs), g
            assert any(c.f32 and c.acc and c.bias for c in cs), g


def test_coverage_of_the_other_entry_points():
    gr = [c for c in G.CASES if c.group == "grouped"]
    assert {(c.layout, c.groups, bool(c.splits), c.acc) for c in gr if c.regime == "exact"} == \
        {(lay, g, sp, acc) for lay in (0, 2) for g in (1, 3, 8) for sp in (False, True) for acc in (0, 1)}
    assert all(c.K < 1024 or c.splits for c in gr) and any(c.regime == "gauss" for c in gr)
    lo = [c for c in G.CASES if c.group == "lora"]
    assert {c.K2 for c in lo} == {8, 16, 128} and {c.res for c in lo} == {None, "bf16", "f32"}
    assert all((c.K % 64 != 0) == (c.regime == "exact256") for c in lo) and all(c.ldu > c.K2 for c in lo)
    assert [p.joint for p in G.PAIRS] == [True, True, False, False] and [p.acc for p in G.PAIRS] == [0, 0, 1, 0]


def test_exact_regime_tests_the_rounding():
    """at K = 4096 a large share of the exact results is not representable in bf16, exact ties among them"""
    c, inp, rows, cols, exp = prepared("gensplit-nt-300x264x4096-exact")
    ref = exp.ref.double()
    r = ref.to(G.BF16).double()
    inexact = r != ref
    assert float(inexact.double().mean()) > 0.3
    assert int(_ties(ref).sum()) > 50


# ---------------------------------------------------------------------------------------------------- planted faults
def _bits16(t):
    return t.view(torch.int16)


def _ulp_step(x):
    """the next bf16 away from zero"""
    return _bits16(x.clone().contiguous()).add_(1).view(G.BF16)


def _ties(ref):
    """elements of a float64 tensor that lie exactly half way between two neighbouring bf16 values"""
    lo = ref.to(G.BF16)                                   # the nearest
    mag = lo.abs().contiguous()
    step = torch.where(ref.abs() > mag.double(), torch.ones_like(_bits16(mag)), -torch.ones_like(_bits16(mag)))
    other = (_bits16(mag) + step).view(G.BF16).double()   # the neighbour on the other side of |ref|
    return (ref != lo.double()) & ((ref.abs() - mag.double()).abs() == (other - ref.abs()).abs())


FAULT_CASES = ["gensplit-nt-300x264x4096-exact-bias-res-acc-a0.5", "gensplit-nt-300x264x4096-gauss-act0",
               "gensplit-nt-300x264x4096-gauss-act1-bias", "ring-nt-200x136x72-exact-bias-res-acc-a0.5",
               "tile256-nt-2824x4104x72-exact-f32-acc-bias"]
ROW_CASES = [n for n in FAULT_CASES if G.BY_NAME[n].M > 256]
EXACT_BF16 = "gensplit-nt-300x264x4096-exact"


def _rejected(name, b, after, exp):
    with pytest.raises(AssertionError):
        G.check(name, after, b, exp)


def _emulated(name, case=(), **ops):
    """the emulation of the case with fields of the case / operands changed -> (Buf, faulty flat buffer, the UNCHANGED case's Exp)"""
    c, inp, rows, cols, exp = prepared(name)
    c2, inp2 = G.Case(c, **dict(case)), dict(inp, **ops)
    b, after = G.place(c, inp, G.emulate(c2, inp2, rows, cols), rows, cols)
    return b, after, exp


def test_one_bf16_ulp_off_is_rejected_in_the_exact_regime():
    c, inp, rows, cols, exp = prepared(EXACT_BF16)
    b, after = G.place(c, inp, G.emulate(c, inp))
    G.check(EXACT_BF16, after, b, exp)
    for r, col in ((0, 0), (127, 255), (299, 263)):
        f = after.clone()
        lo = G.logical(b, f)
        lo[r, col] = _ulp_step(lo[r, col].reshape(1))[0]
        _rejected(EXACT_BF16, b, f, exp)


def test_a_tie_rounded_up_instead_of_to_even_is_rejected():
    c, inp, rows, cols, exp = prepared(EXACT_BF16)
    ref = exp.ref.double()
    good = ref.to(G.BF16)
    tie = _ties(ref) & (good.double().abs() < ref.abs())           # ties that round-to-nearest-even sends DOWN (towards zero)
    assert int(tie.sum()) > 10
    b, after = G.place(c, inp, G.emulate(c, inp))
    r, col = tie.nonzero()[0].tolist()
    lo = G.logical(b, after)
    assert lo[r, col] == good[r, col]
    lo[r, col] = _ulp_step(good[r, col].reshape(1))[0]            # round-half-away
    assert abs(float(lo[r, col]) - float(ref[r, col])) == abs(float(good[r, col]) - float(ref[r, col]))      # as close as the right answer
    _rejected(EXACT_BF16, b, after, exp)


@pytest.mark.parametrize("name", FAULT_CASES)
def test_last_k_chunk_dropped_is_rejected(name):
    c, inp, rows, cols, exp = prepared(name)
    A = inp["A"]
    f = A.flat.clone()
    a = G.logical(A, f)
    if c.layout == 2:
        a[c.K - 8:] = 0
    else:
        a[:, c.K - 8:] = 0
    _rejected(name, *_emulated(name, A=G.Buf(f, A.off, A.rows, A.width, A.ld)))


@pytest.mark.parametrize("name", ROW_CASES)
@pytest.mark.parametrize("edge", [128, 256])
def test_rows_swapped_across_a_tile_boundary_are_rejected(name, edge):
    c, inp, rows, cols, exp = prepared(name)
    out = G.emulate(c, inp, rows, cols)
    if rows is None:
        i, j = edge - 1, edge
    else:
        i, j = rows.tolist().index(edge - 1), rows.tolist().index(edge)
    out[[i, j]] = out[[j, i]]
    b, after = G.place(c, inp, out, rows, cols)
    _rejected(name, b, after, exp)


@pytest.mark.parametrize("name", FAULT_CASES)
def test_epilogue_faults_are_rejected(name):
    c, inp, rows, cols, exp = prepared(name)
    if c.bias:
        _rejected(name, *_emulated(name, case={"bias": 0}))                                 # bias omitted
        if c.alpha != 1.0:                                                         # alpha applied after the bias: alpha (acc + bias)
            bb = inp["bias"]
            f = bb.flat.clone()
            G.logical(bb, f)[:] = (G.logical(bb).float() * c.alpha).to(G.BF16)
            _rejected(name, *_emulated(name, bias=G.Buf(f, bb.off, bb.rows, bb.width, bb.ld)))
    if c.acc:                                                                      # the accumulate term added twice
        out = G.emulate(c, inp, rows, cols).float() + G._sub(G.logical(inp["C"]), rows, cols).float()
        b, after = G.place(c, inp, out, rows, cols)
        _rejected(name, b, after, exp)
    if c.res:
        _rejected(name, *_emulated(name, case={"res": None}))


@pytest.mark.parametrize("name", FAULT_CASES)
def test_stray_stores_and_nan_are_rejected(name):
    c, inp, rows, cols, exp = prepared(name)
    b, after = G.place(c, inp, G.emulate(c, inp, rows, cols), rows, cols)
    G.check(name, after, b, exp)
    for cell in (b.off - 1, 0, b.off + b.rows * b.ld, after.numel() - 1):          # one guard cell written
        f = after.clone()
        f[cell] = 0.0
        _rejected(name, b, f, exp)
    for r in (0, b.rows - 1):                                                      # one padding column of C written
        for col in (b.width, b.ld - 1):
            f = after.clone()
            f[b.off + r * b.ld + col] = 1.0
            _rejected(name, b, f, exp)
    f = after.clone()                                                              # a NaN in the result
    G.logical(b, f)[b.rows // 2, b.width // 2] = float("nan")
    _rejected(name, b, f, exp)
