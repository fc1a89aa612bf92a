"""The checker of tests/fused_gemm_ref.py, on the CPU: for every case of tests/test_hip_fused_gemm_edges.py the fp32 emulation of the
route passes the checker (bitwise where the exact regimes promise bits; the multi-tile cases on a row sample that holds every tile edge,
with all columns), the case table meets the entry points' alignment rules and records the route their launch predicates give, and each
planted fault is rejected on the smallest case where it can show."""
import functools

import pytest
import torch

from tests import fused_gemm_ref as R

IDS = [c.name for c in R.CASES]
F32, BF16 = torch.float32, torch.bfloat16


@functools.lru_cache(maxsize=4)
def prepared(name):
    c = R.BY_NAME[name]
    inp = R.make(c)
    rows = R.sample(c)
    return c, inp, rows, R.expect(c, inp, "cpu", rows)


def placed(c, inp, rows, outs):
    """-> ({name: Buf}, {name: flat after}) for a call that wrote `outs` ({name: logical tensor}); untouched outputs keep their content"""
    bufs, after = {}, {}
    for n in R.outputs(c):
        old = R.logical(inp[n]) if rows is None else R.logical(inp[n])[rows]
        bufs[n], after[n] = R.place(c, inp, n, outs.get(n, old), rows)
    return bufs, after


def verdict(c, inp, rows, exp, outs, stray=None):
    bufs, after = placed(c, inp, rows, outs)
    if stray:
        stray(bufs, after)
    R.check_case(c, dict(inp, **bufs), after, exp)


def rejected(*a, **k):
    with pytest.raises(AssertionError):
        verdict(*a, **k)


@pytest.mark.parametrize("name", IDS)
def test_fp32_emulation_passes_its_checker(name):
    c, inp, rows, exp = prepared(name)
    verdict(c, inp, rows, exp, R.emulate(c, inp, rows))


def predicted_fused(c):
    """the launch predicates of vlr_gemm256p_fused_try_launch / _seg_try_launch / _swiglu_bwd_try_launch and the dispatchers' own
    conditions (csrc/gemm.hip), on aligned operands"""
    if c.K < 256 or (c.r and c.K % 64):
        return False
    if c.op == "rope":
        inner = [b for b in c.blocks if b < c.N]
        return c.hd == 128 and c.bias in (None, 0, 4) and c.N % 256 == 0 and c.rope_cols % 256 == 0 and all(b % 256 == 0 for b in inner)
    return True


@pytest.mark.parametrize("name", IDS)
def test_case_table_is_aligned_and_records_its_route(name):
    c = R.BY_NAME[name]
    assert c.n256 == (1 if predicted_fused(c) else 0)
    assert c.K % 8 == 0 and c.N % 8 == 0 and c.M > 0
    assert R.fused(c) or c.regime != "gauss"                      # a fallback's rounded intermediate is determined in the exact regimes only
    if c.op != "bwd":
        assert c.ldx > c.K and c.ldx % 8 == 0
    if c.r:
        assert c.r % 8 == 0 and c.ldu % 8 == 0 and c.ldu > len(c.blocks) * c.r and c.blocks[-1] == c.N
    if c.op == "rope":
        assert c.rope_cols % c.hd == 0 and c.rope_cols <= c.N and c.hd % 16 == 0
    inp = R.make(c)
    for k, b in inp.items():                                       # every [M][.] buffer has NaN rows behind row M, every buffer NaN guards
        if k == "pos":
            continue
        assert bool(torch.isnan(b.flat[:b.off]).all()) and bool(torch.isnan(b.flat[b.off + b.rows * b.ld:]).all()), k
        if k in ("x", "u", "dy", "gu", "act", "qkv", "ws", "add"):
            assert b.flat.numel() >= b.off + (c.M + R.GUARD_ROWS) * b.ld + R.GUARD, k
        if b.ld > b.width:
            assert bool(torch.isnan(b.flat[b.off + b.width:b.off + b.ld]).all()), k


def test_coverage_rules():
    by = lambda op, **kw: [c for c in R.CASES if c.op == op and all(c[k] == v for k, v in kw.items())]      # noqa: E731
    sw = by("swiglu", r=0)
    assert {(c.M, c.I, c.K) for c in sw} >= {(8, 8, 256), (264, 136, 264), (37, 128, 320), (549, 520, 256), (300, 136, 200), R.MULTI["swiglu"]}
    for shape in ((8, 8, 256), (264, 136, 264), (37, 128, 320), (549, 520, 256), (300, 136, 200)):
        assert {c.store_gu for c in sw if (c.M, c.I, c.K) == shape and c.regime == "exact"} == {0, 1}, shape
    rp = by("rope", r=0)
    assert {(c.M, c.K, c.N, c.rope_cols) for c in rp} >= {(8, 256, 768, 512), (264, 264, 1024, 768), (37, 256, 256, 256), (8, 256, 768, 0),
                                                         (300, 256, 384, 256), (37, 200, 768, 512), (4104, 256, 4352, 4096)}
    assert any(c.hd == 64 and c.n256 == 0 for c in rp)
    assert {c.bias for c in rp if c.n256 == 1} == {None, 0, 4} and any(c.bias == 1 and c.n256 == 0 for c in rp)
    bw = by("bwd")
    assert {(c.M, c.I, c.K) for c in bw} >= {(8, 8, 256), (264, 264, 264), (37, 512, 256), (549, 520, 256), (549, 520, 128), R.MULTI["bwd"]}
    assert {(c.add, c.n256) for c in bw} >= {(a, n) for a in (None, "sep", "alias") for n in (0, 1)}
    lo = [c for c in R.CASES if c.r]
    for op in ("swiglu", "rope"):
        mine = [c for c in lo if c.op == op]
        assert {c.r for c in mine if c.n256} == {8, 128} and any(c.regime == "gauss" for c in mine)
        assert any(c.regime == "exact256" and c.n256 == 0 for c in mine)
    assert {len(c.blocks) for c in lo if c.op == "rope" and c.n256} == {1, 3}
    assert any(c.op == "rope" and c.n256 == 0 and c.K % 64 == 0 and c.blocks[0] % 256 for c in lo)      # refused for its q_cols alone
    for op in ("swiglu", "rope", "bwd"):
        assert any(R.is_multi(c) and c.op == op and c.regime == "exact" for c in R.CASES), op
        assert {c.regime for c in R.CASES if c.op == op} >= {"exact", "gauss"}, op


def test_positions_and_tables():
    for M in (8, 37, 264, 4104):
        p = R.positions(M, 3).tolist()
        assert {0, R.MAX_POS - 1, -1, R.MAX_POS, 2 ** 30} <= set(p) and p[2] == p[3] and p[4] < p[3]
    p = R.positions(264, 3)
    assert bool((p[100:139] > p[101:140]).all())                   # the descending run
    cos, sin = R.planted_tables(64)
    allowed = {0.0, 0.25, 0.5, 1.0, 2.0}
    assert set(cos.abs().unique().tolist()) <= allowed and set(sin.abs().unique().tolist()) <= allowed
    both = torch.cat([cos, sin], 1)
    assert len({tuple(r) for r in both.tolist()}) == R.MAX_POS       # no two positions share their table rows
    assert float((both[:, :-1] != both[:, 1:]).float().mean()) > 0.7 and not torch.equal(cos, sin)


def test_exact_regime_tests_the_rounding():
    """a large share of the exact gate | up and q | k | v results is not representable in bf16"""
    for name in ("swiglu-549x520x256-exact-gu1", "rope-264x264x4+2-exact-hd128-rc768"):
        c, inp, rows, exp = prepared(name)
        ref = exp["gu" if c.op == "swiglu" else "qkv"].ref.double()
        assert float((ref.to(BF16).double() != ref).double().mean()) > 0.3, name


def test_fused_tail_peel_is_never_chosen():
    """choose_peel(..., tail256 = true) restated: no M, tile-row width or CU count peels a tile row (module docstring)"""
    assert all(R.peel_tail256_best(M, tn, ncu) == 0 for ncu in (64, 240, 256) for tn in (1, 2, 7, 16, 17, 43, 86) for M in range(256, 66000, 128))


# ---------------------------------------------------------------------------------------------------- planted faults
SW = "swiglu-8x8x256-exact-gu1"
SW0 = "swiglu-8x8x256-exact-gu0"
SW_EDGE = "swiglu-264x136x264-exact-gu1"
SW_BIG = "swiglu-549x520x256-exact-gu1"
RP = "rope-8x256x2+2-exact-hd128-rc512"
RPB = "rope-8x256x2+2-exact-hd128-rc512-bias0"
RP_GQA = "rope-264x264x4+2-exact-hd128-rc768-bias0"
BW = "bwd-8x8x256-exact"
BW_ADD = "bwd-264x264x264-exact-addsep"
BW_ALIAS = "bwd-264x264x264-exact-addalias"


def _with(inp, key, fn):
    """inp with the logical content of operand `key` replaced by fn(old)"""
    b = inp[key]
    f = b.flat.clone()
    R.logical(b, f)[:] = fn(R.logical(b).clone())
    return dict(inp, **{key: R.Buf(f, b.off, b.rows, b.width, b.ld)})


@pytest.mark.parametrize("name", [SW, SW0, "swiglu-264x136x264-gauss-gu1"])
def test_gate_and_up_halves_swapped_are_rejected(name):
    c, inp, rows, exp = prepared(name)
    rejected(c, inp, rows, exp, R.emulate(c, _with(inp, "W", lambda w: torch.cat([w[c.I:], w[:c.I]]))))


@pytest.mark.parametrize("name", [SW_EDGE, "swiglu-264x136x264-exact-gu0"])
def test_up_read_at_the_padded_column_offset_is_rejected(name):
    """up column j taken from column 128 ceil(I / 128) + j of the product (zero past 2 I) instead of I + j"""
    c, inp, rows, exp = prepared(name)
    off = -(-c.I // 128) * 128

    def shifted(w):
        up = torch.zeros(c.I, c.K, dtype=w.dtype)
        n = max(0, 2 * c.I - off)
        up[:n] = w[off:off + n]
        return torch.cat([w[:c.I], up])
    rejected(c, inp, rows, exp, R.emulate(c, _with(inp, "W", shifted)))


def test_act_from_the_rounded_gate_up_is_rejected_on_the_fused_route():
    c, inp, rows, exp = prepared(SW_BIG)
    outs = R.emulate(c, inp)
    R.check(SW_BIG, *_one(c, inp, "act", outs["act"]), exp["act"])
    gu = outs["gu"].float()
    twice = (gu[:, :c.I] * torch.sigmoid(gu[:, :c.I]) * gu[:, c.I:]).to(BF16)
    rejected(c, inp, rows, exp, dict(outs, act=twice))


def _one(c, inp, name, out):
    b, f = R.place(c, inp, name, out)
    return f, b


def rope_faulty(c, inp, partner=False, sine=1.0, next_row=False, bias_after=(), rotate_v=False, wrap=False):
    """the fused route's fp32 emulation with one fault planted.  bias_after: the heads whose bias is added after the rotation"""
    N, hd, half = c.N, c.hd, c.hd // 2
    acc, _ = R.accum(c, inp, F32)
    late = None
    if c.bias is not None:
        bias = R.logical(inp["bias"]).float()
        if bias_after:
            late = torch.zeros(1, N)
            for h in bias_after:
                late[:, h * hd:(h + 1) * hd] = bias[:, h * hd:(h + 1) * hd]
            bias = bias - late
        acc = acc + bias
    pos = inp["pos"].long()
    if next_row:
        pos = torch.cat([pos[1:], pos[-1:]])
    p = pos % R.MAX_POS if wrap else pos.clamp(0, R.MAX_POS - 1)
    cs, sn = R.logical(inp["cos"])[p][:, None, :], sine * R.logical(inp["sin"])[p][:, None, :]
    rc = N if rotate_v else c.rope_cols
    h = acc[:, :rc].reshape(c.M, rc // hd, hd)
    x1, x2 = h[..., :half], h[..., half:]
    p1, p2 = (h[..., 1:half + 1], torch.roll(h, -1, -1)[..., half:]) if partner else (x2, x1)
    y = acc.clone()
    y[:, :rc] = torch.cat([x1 * cs - p1 * sn, x2 * cs + p2 * sn], -1).reshape(c.M, rc)
    return {"qkv": (y if late is None else y + late).to(BF16)}


@pytest.mark.parametrize("name", [RP, RPB, RP_GQA])
def test_rope_faults_are_rejected(name):
    c, inp, rows, exp = prepared(name)
    good = rope_faulty(c, inp)
    assert torch.equal(R.row_bits(good["qkv"]), R.row_bits(R.emulate(c, inp)["qkv"]))        # without a fault: the emulation
    verdict(c, inp, rows, exp, good)
    for fault in (dict(partner=True), dict(sine=-1.0), dict(next_row=True), dict(rotate_v=True), dict(wrap=True)):
        rejected(c, inp, rows, exp, rope_faulty(c, inp, **fault))
    if c.bias is not None:
        for h in range(c.rope_cols // c.hd):           # on every rotated head with a bias: the dwarfing, the vanishing and the like-sized one
            if float(R.logical(inp["bias"])[:, h * c.hd:(h + 1) * c.hd].abs().max()) > 0:
                rejected(c, inp, rows, exp, rope_faulty(c, inp, bias_after=(h,)))


def test_the_wrapped_position_shows_in_each_out_of_range_row():
    """rows 5, 6, 7 hold -1, MAX_POS and 2^30: each alone is rejected when wrapped instead of clamped"""
    c, inp, rows, exp = prepared(RP)
    good, bad = rope_faulty(c, inp)["qkv"], rope_faulty(c, inp, wrap=True)["qkv"]
    for r in (5, 6, 7):
        out = good.clone()
        out[r] = bad[r]
        rejected(c, inp, rows, exp, {"qkv": out})


@pytest.mark.parametrize("name", [SW, SW0, RP, BW, SW_EDGE, RP_GQA, BW_ADD])
def test_last_eight_columns_unwritten_are_rejected(name):
    c, inp, rows, exp = prepared(name)
    outs = R.emulate(c, inp)
    for n in outs:
        if bool(torch.isnan(outs[n]).all()):
            continue
        o = outs[n].clone()
        o[:, -8:] = R.logical(inp[n])[:, -8:]                       # what the buffer held before the call
        rejected(c, inp, rows, exp, dict(outs, **{n: o}))
        if c.op != "rope":                                         # the last eight columns of the gate half too
            o = outs[n].clone()
            h = o.shape[1] // 2 if n == "gu" else o.shape[1]
            o[:, h - 8:h] = R.logical(inp[n])[:, h - 8:h]
            rejected(c, inp, rows, exp, dict(outs, **{n: o}))


@pytest.mark.parametrize("name", [SW, SW0, RP, BW, BW_ADD, BW_ALIAS, "swiglu-300x136x200-exact-gu0", "bwd-549x520x128-exact"])
def test_row_M_written_is_rejected(name):
    """one cell of row M (a guard row) written, in every buffer the call may write - the scratch ones included"""
    c, inp, rows, exp = prepared(name)
    outs = R.emulate(c, inp)
    verdict(c, inp, rows, exp, outs)
    for n in R.outputs(c):
        for col in (0, inp[n].width - 1):
            def stray(bufs, after, n=n, col=col):
                b = bufs[n]
                after[n][b.off + b.rows * b.ld + col] = 1.0
            rejected(c, inp, rows, exp, outs, stray=stray)
        for cell in (0, inp[n].off - 1, inp[n].flat.numel() - 1):
            def stray(bufs, after, n=n, cell=cell):
                after[n][cell] = 0.0
            rejected(c, inp, rows, exp, outs, stray=stray)


@pytest.mark.parametrize("name", [SW0, "swiglu-264x136x264-gauss-gu0"])
def test_gu_written_without_store_gu_is_rejected(name):
    c, inp, rows, exp = prepared(name)
    stored = R.emulate(R.Case(c, store_gu=1), inp)
    rejected(c, inp, rows, exp, stored)
    one = torch.full_like(stored["gu"], float("nan"))
    one[c.M - 1, 2 * c.I - 1] = stored["gu"][c.M - 1, 2 * c.I - 1]      # a single cell
    rejected(c, inp, rows, exp, dict(stored, gu=one))


@pytest.mark.parametrize("name", [BW_ADD, BW_ALIAS, "bwd-549x520x128-exact-addsep", "bwd-549x520x256-gauss-addsep"])
def test_addend_dropped_is_rejected(name):
    c, inp, rows, exp = prepared(name)
    key = "add" if c.add == "sep" else "ws"
    rejected(c, inp, rows, exp, R.emulate(c, _with(inp, key, torch.zeros_like)))


@pytest.mark.parametrize("name", [BW, BW_ADD, "bwd-264x264x264-gauss"])
def test_dgate_and_dup_exchanged_are_rejected(name):
    c, inp, rows, exp = prepared(name)
    o = R.emulate(c, inp)["gu"]
    rejected(c, inp, rows, exp, {"gu": torch.cat([o[:, c.I:], o[:, :c.I]], 1)})


@pytest.mark.parametrize("name", [SW, RP, BW])
def test_nan_and_one_ulp_are_rejected(name):
    c, inp, rows, exp = prepared(name)
    outs = R.emulate(c, inp)
    n = R.outputs(c)[0]
    o = outs[n].clone()
    o[c.M // 2, 3] = float("nan")
    rejected(c, inp, rows, exp, dict(outs, **{n: o}))
    if R.bitwise(c, n):
        o = outs[n].clone()
        cell = o[c.M - 1, -1:].clone()
        o[c.M - 1, -1] = cell.view(torch.int16).add_(1).view(BF16)[0]      # the next bf16
        rejected(c, inp, rows, exp, dict(outs, **{n: o}))
