"""The checker of tests/lora_ref.py on the CPU (no GPU, no marker): for every case the fp32 emulation passes against the float64
reference; the exact regime's magnitude and "kept and dropped in every byte column" assertions hold (make() asserts them); the packed
layouts round-trip and match the formulas of include/vlr.h one element at a time; the row-set helpers' references agree with a plain
loop; and the checker REJECTS each planted fault - a keep bit flipped, a target's block at t * r instead of t * ustride, the last K step
dropped, a nonzero element in an unmarked row, a write into the padding, a write to a row >= M, alpha applied twice, a tie rounded away
from even."""
import pytest
import torch

from tests import lora_ref as L


@pytest.mark.parametrize("name", [c.name for c in L.CASES])
def test_emulation_passes_the_checker(name):
    c = L.BY_NAME[name]
    inp = L.make(c)                       # asserts sum |terms| < 2^24 and the mixed masks (exact regime)
    e = L.expect(c, inp)
    L.verify(c, L.place(c, inp, L.emulate(c, inp)), inp, e)
    if c.regime == "exact":
        assert e.rel is None and bool((e.ref.double() == L.formula(c, inp, L.F64)[0]).all())      # float64 -> float32 lost nothing


def test_case_table_covers_the_templates():
    u = [c for c in L.CASES if c.kind == "u"]
    for r, steps in ((64, (1, 2, 4, 5, 6, 7, 13)), (128, (1, 2, 4, 5, 6, 7, 13)), (256, (1, 2, 3, 4, 5, 9))):
        assert {c.inn // 64 for c in u if c.r == r} >= set(steps)
        assert {c.M for c in u if c.r == r} >= {1, 63, 64, 65, 129, 513, 577}
        assert {c.n for c in u if c.r == r} >= {1, 3, 4}
    assert any(c.r == 256 and c.n * 2 == L.LR_MAXT for c in u) and any(c.M == 1025 and c.r == 256 for c in u)
    dx = [c for c in L.CASES if c.kind == "dx"]
    assert {(c.n, c.r) for c in dx if L.dx_streams(c) and L.dx_slab(c) == 64} >= {(n, r) for n in (1, 2, 3) for r in (64, 128)} | {(2, 256)}
    assert {(c.n, c.r) for c in dx if c.inn == 8192 and L.dx_slab(c) == 128} == {(1, 64), (3, 64), (2, 128)}
    assert {c.inn for c in dx if (c.n, c.r) == (1, 256) and L.dx_slab(c) == 128} >= {128, 256}
    assert any(not L.dx_streams(c) and c.r == 16 for c in dx) and any(not L.dx_streams(c) and c.inn == 136 for c in dx)
    assert any(not L.dx_streams(c) and c.n == 5 for c in dx) and any(not L.dx_streams(c) and (c.n, c.r) == (3, 256) for c in dx)
    walk = [c for c in dx if "walk" in c.name]
    assert all(L.dx_ranges(c) == [2, 2, 2, 1] and L.dx_ranges(c, 128) == [3, 3, 1] and c.n >= 2 and c.masked for c in walk)
    assert {c.acc for c in walk} == {0, 1} and any(c.comm_cus == 128 for c in walk)
    g = [c for c in L.CASES if c.kind == "grp"]
    assert {c.K for c in g if c.mask_on == 1} >= {64, 72, 128, 1024, 1088}
    assert {c.K for c in g if c.mask_on in (2, 3) and c.ktl is None} >= {8, 63, 64, 65, 130, 1024, 1100}
    assert {c.splits for c in g if c.K in (1024, 1088, 1100)} == {4} and all(c.splits == 0 for c in g if c.K < 1024)


# ---------------------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("rows", L.BITS2_ROWS)
@pytest.mark.parametrize("cols", L.BITS2_COLS)
def test_packed_layouts_round_trip(rows, cols):
    keep = L.keep_mask(99 + rows + cols, rows, cols, 0.25)
    assert 0 < int(keep.sum()) < keep.numel()
    rm, kt = L.pack_rowmajor(keep), L.pack_kt(keep)
    assert rm.numel() == rows * cols // 8 and kt.numel() == L.kt_bytes(rows, cols)
    assert torch.equal(L.unpack_rowmajor(rm, rows, cols), keep) and torch.equal(L.unpack_kt(kt, rows, cols), keep)
    for row in sorted({0, rows - 1, rows // 2, min(rows - 1, 63), min(rows - 1, 64), min(rows - 1, 7), min(rows - 1, 8)}):
        for col in sorted({0, cols - 1, cols // 2, 7, min(cols - 1, 8)}):
            i = row * cols + col                                   # include/vlr.h: bit e of byte i = element 8 i + e
            assert (int(rm[i // 8]) >> (i % 8)) & 1 == int(keep[row, col])
            byte, bit = L.kt_byte_of(row, col, cols)               # byte ((row / 64) * cols + col) * 8 + (row % 64) / 8, bit = row % 8
            assert (int(kt[byte]) >> bit) & 1 == int(keep[row, col])
    popcount = sum(bin(int(b)).count("1") for b in kt.tolist())
    assert popcount == int(keep.sum())                             # the rows past the last one are zero


def test_row_set_references_agree_with_a_plain_loop():
    for M in (1, 63, 64, 65, 385, 4097):
        for kind in ("sparse", "dense", "lasttile", "zero"):
            m = L.helper_row_set(M, kind)
            tiles = [t for t in range(-(-M // 64)) if any(int(m[r]) for r in range(t * 64, min(M, t * 64 + 64)))]
            assert L.tile_list(m, M) == [len(tiles)] + tiles
            for tr in (64, 128, 300):
                flags = [0 if any(int(m[r]) for r in range(t * tr, min(M, t * tr + tr))) else 1 for t in range(-(-M // tr))]
                assert L.tile_flags(m, M, tr).tolist() == flags
    assert L.helper_row_set(8200, "sparse")[64 * 64:].any()         # marks past the 64th tile: the second ballot round


# ---------------------------------------------------------------------------------------------------- planted faults
def _first(pred):
    """the first case per (family, regime) that satisfies pred and is small"""
    seen, out = set(), []
    for c in L.CASES:
        k = (L.family(c), c.regime)
        if k not in seen and c.M <= 1100 and c.inn <= 1024 and pred(c):
            seen.add(k)
            out.append(c)
    return out


def _rejects(c, inp, e, after, what):
    with pytest.raises(AssertionError):
        L.verify(c, after, inp, e)
    L.verify(c, L.place(c, inp, L.emulate(c, inp)), inp, e)          # ... and the unspoilt emulation still passes
    assert what


def _flip_position(c, inp):
    """(row, col) of target 0's mask whose flip moves the output most"""
    x, W = torch.nan_to_num(L.logical(inp["x"]).float()), torch.nan_to_num(L.logical(inp["A"]).float())
    if c.kind in ("dx", "dx1"):
        w = (x[:, :c.r] @ W[:c.r]).abs()
    elif c.kind == "grp" and c.layout == 2:
        w = W.abs() * x[:, :c.Mo].abs().amax(1, keepdim=True)
    else:
        rows = c.r if c.kind == "u" else c.N
        w = x.abs() * W[:rows].abs().amax(0, keepdim=True)
        if inp["rowmask"] is not None:
            w = w * inp["rowmask"].bool()[:, None]
    i, j = divmod(int(w.argmax()), w.shape[1])
    assert float(w[i, j]) > 0
    return i, j


FLIP = _first(lambda c: c.masked and c.rowmask != "zero" and c.get("ktl") != "empty")


@pytest.mark.parametrize("name", [c.name for c in FLIP])
def test_rejects_a_flipped_keep_bit(name):
    c = L.BY_NAME[name]
    inp = L.make(c)
    i, j = _flip_position(c, inp)
    _rejects(c, inp, L.expect(c, inp), L.place(c, inp, L.emulate(c, inp, fault=("flip", 0, i, j))), "flip")


def test_flip_covers_every_masked_family():
    assert {L.family(c) for c in FLIP} == {L.family(c) for c in L.CASES if c.masked}


@pytest.mark.parametrize("name", [c.name for c in _first(lambda c: c.kind == "u" and c.ustride != c.r and c.n >= 2)])
def test_rejects_a_block_at_t_times_r(name):
    c = L.BY_NAME[name]
    inp = L.make(c)
    wrong = torch.arange(c.n * c.r)                                  # target t at t * r instead of t * ustride
    _rejects(c, inp, L.expect(c, inp), L.place(c, inp, L.emulate(c, inp), cols=wrong), "block")


KSTEP = _first(lambda c: c.Kc >= 128 and c.rowmask != "zero" and c.get("ktl") in (None, "all", "gap") and not (c.kind == "v" and c.outs[-1] < 128))


@pytest.mark.parametrize("name,fault", [(c.name, f) for c in KSTEP for f in ("lastk", "alpha2") if not (f == "alpha2" and c.kind == "v")])      # (v has no alpha)
def test_rejects_a_dropped_k_step_and_alpha_twice(name, fault):
    c = L.BY_NAME[name]
    inp = L.make(c)
    _rejects(c, inp, L.expect(c, inp), L.place(c, inp, L.emulate(c, inp, fault=fault)), fault)


ROWSET = _first(lambda c: c.rowmask in ("gap", "ragged") and c.kind in ("u", "v", "grp"))


@pytest.mark.parametrize("name", [c.name for c in ROWSET])
def test_rejects_a_nonzero_element_in_an_unmarked_row(name):
    c = L.BY_NAME[name]
    inp = L.make(c)
    after = L.place(c, inp, L.emulate(c, inp))
    row = int((inp["rowmask"] == 0).nonzero()[-1])
    assert float(L.logical(inp["out"], after)[row, 0]) == 0.0
    L.logical(inp["out"], after)[row, 0] = 2.0 ** -20
    _rejects(c, inp, L.expect(c, inp), after, "unmarked row")


def _places(c):
    """where a stray write can land: between the targets' blocks only when ustride > r; dx has no leading dimension (dense rows)"""
    return ["row>=M", "front guard"] + (["between blocks"] if c.kind == "u" else []) + ([] if c.kind in ("dx", "dx1") else ["padding"])


OUTSIDE = _first(lambda c: c.get("ustride", 0) != c.r if c.kind == "u" else True)


@pytest.mark.parametrize("name,where", [(c.name, w) for c in OUTSIDE for w in _places(c)])
def test_rejects_a_write_outside_the_result(name, where):
    c = L.BY_NAME[name]
    inp = L.make(c)
    b = inp["out"]
    after = L.place(c, inp, L.emulate(c, inp))
    if where == "between blocks":
        cell = b.off + c.r                                           # the first column behind target 0's block
    elif where == "padding":
        assert b.ld > b.width
        cell = b.off + (b.rows - 1) * b.ld - 1                       # the last padding cell of the last row but one ... or of row 0
        cell = cell if b.rows > 1 else b.off + b.width
    elif where == "row>=M":
        cell = b.off + b.rows * b.ld
    else:
        cell = b.off - 1
    assert bool(torch.isnan(after[cell]))
    after[cell] = 0.0
    _rejects(c, inp, L.expect(c, inp), after, where)


def test_rejects_a_tie_rounded_away_from_even():
    """exact regime: an expected value exactly between two bf16 numbers goes to the even one; the other neighbour is one ulp off"""
    found = 0
    for c in L.CASES:
        if c.regime != "exact" or c.M > 1100 or c.inn > 1024 or found >= 6:
            continue
        inp = L.make(c)
        e = L.expect(c, inp)
        bits = e.ref.contiguous().view(torch.int32)
        tie = ((bits & 0xFFFF) == 0x8000).nonzero()
        if not len(tie):
            continue
        found += 1
        i, j = tie[0].tolist()
        hi = int(bits[i, j]) >> 16                                   # truncated: the neighbour towards zero (sign-magnitude)
        good, wrong = hi + (hi & 1), hi + 1 - (hi & 1)
        after = L.place(c, inp, L.emulate(c, inp))
        cols = L.out_cols(c)
        cell = L.logical(inp["out"], after)[i:i + 1, (j if cols is None else int(cols[j]))]
        assert int(cell.view(torch.int16)) & 0xFFFF == good & 0xFFFF
        cell.view(torch.int16)[...] = wrong - (1 << 16) if wrong >= (1 << 15) else wrong
        _rejects(c, inp, e, after, "tie")
    assert found >= 3, "the exact cases hold too few ties to test the tie rule"
