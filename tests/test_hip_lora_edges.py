"""The LoRA / PLoRA adapter products (csrc/lora_rows.hip, csrc/lora_dx.hip, the masked and grouped paths of csrc/gemm.hip and
csrc/gemm128p.hip) and their helpers element by element at their loop edges: every case of tests/lora_ref.py through the C ABI against
the float64 reference - bitwise in the exact regime, an elementwise bound in the gauss regime - with keep masks packed on the host from
the oracle's mask, NaN in every operand's padding and in every row the contract says is not read, NaN guards around every buffer, the
whole flat output compared cell by cell, the routes that have an observable asserted from it (writes into a NaN-filled split-K workspace,
NaN left in place by a tile that is not computed) and every case run twice for bit-identical results.
tests/test_lora_checker_host.py runs the same checker on the CPU.  Needs a real MI355X: pytest -m gpu"""
import ctypes as C

import pytest
import torch

from tests import lora_ref as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
WS_BYTES = 64 << 20


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return _hip


def restore(hip):
    hip.ensure_splitk_workspace(force=True)
    hip.helper("vlr_set_comm_cus", -1)


class Run:
    """one case on the GPU: the operands with their NaN padding and guards (g), the entry point's arguments"""

    def __init__(self, c):
        self.c = c
        self.inp = L.make(c)
        self.g = {k: b.flat.to(DEV) for k, b in self.inp.items() if isinstance(b, L.Buf)}
        self.rowmask = None if self.inp["rowmask"] is None else self.inp["rowmask"].to(DEV)
        self.c0 = self.g["out"].clone()
        self.ktl = None

    def at(self, k):
        return self.g[k][self.inp[k].off:] if k in self.g else None

    def launch(self, hip):
        c, inp = self.c, self.inp
        bits, gs = self.at("bits"), inp.get("gstride", 0)
        x, W, out = self.at("x"), self.at("A"), self.at("out")
        if c.kind == "u":
            hip.call("vlr_lora_rows_u", c.n, x, c.ldx, W, out, c.ldu, c.ustride, c.M, c.inn, c.r, c.alpha, bits, gs, self.rowmask)
        elif c.kind == "v":
            hip.call("vlr_lora_rows_v", c.n, x, c.lddy, (C.c_int * c.n)(*c.outs), W, out, c.ldv, c.M, c.r, self.rowmask)
        elif c.kind == "dx":
            args = (c.n, x, c.ldv, W, out, c.M, c.inn, c.r, c.p, inp["seed"], c.scale, c.acc)
            if c.entry == "multi":
                hip.call("vlr_gemm_dropout_acc_multi", *args)
            elif c.entry == "bits":
                hip.call("vlr_gemm_dropout_acc_multi_bits", *args, bits, gs)
            else:
                hip.call("vlr_gemm_dropout_acc_multi_rows", *args, bits, gs, self.rowmask)
        elif c.kind == "dx1":
            args = (x, c.ldv, W, out, self.at("scratch"), c.M, c.inn, c.r, c.p, inp["seed"], c.scale)
            if c.mode == "bits":
                hip.call("vlr_gemm_dropout_acc_bits", *args, bits)
            else:
                hip.call("vlr_gemm_dropout_acc", *args)
        else:
            lda, ldb, ldc = inp["x"].ld, inp["A"].ld, inp["out"].ld
            if c.layout == 2:
                gA, gB, gC = c.Mo, (0 if c.mask_on else c.No), c.Mo * ldc
            elif c.layout == 0:
                gA, gB, gC = 0, c.N * ldb, c.N
            else:
                gA, gB, gC = c.K, c.K * ldb, c.N
            args = (c.layout, x, W, out, c.Mo, c.No, c.K, lda, ldb, ldc, c.groups, gA, gB, gC, c.alpha, c.acc, c.mask_on, inp["seed"], c.p,
                    c.inn if c.mask_on else 0)
            if c.entry == "grouped":
                hip.call("vlr_gemm_grouped", *args)
            elif c.entry == "bits":
                hip.call("vlr_gemm_grouped_bits", *args, bits, gs)
            elif c.entry == "rows":
                hip.call("vlr_gemm_grouped_bits_rows", *args, bits, gs, self.rowmask)
            else:
                self.ktl = torch.full((c.K // 64 + 2 + 2 * L.GUARD,), L.INT_POISON[torch.int32], dtype=torch.int32, device=DEV)
                hip.call("vlr_rows_tile_list", self.rowmask, c.K, self.ktl[L.GUARD:])
                hip.call("vlr_gemm_grouped_bits_ktiles", *args, bits, gs, self.ktl[L.GUARD:])


def run_case(hip, c, say=print):
    """runs the case twice; asserts the route observables, determinism, the read-only operands, the result and the guards"""
    r = Run(c)
    rows_form = c.kind == "grp" and c.entry == "rows"
    ws = torch.full((WS_BYTES // 4,), NAN, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    results, raw = [], None
    try:
        assert hip.helper("vlr_gemm_set_splitk_workspace", ws.data_ptr(), ws.numel() * 4) == 0
        if c.comm_cus >= 0:
            assert hip.helper("vlr_set_comm_cus", c.comm_cus) == 0
        cus = hip.helper("vlr_compute_cus")
        for i in range(2):
            r.g["out"].copy_(r.c0)
            ws.fill_(NAN)
            r.launch(hip)
            torch.cuda.synchronize()
            if i == 0:
                wrote_ws = bool((~torch.isnan(ws)).any())
                raw = r.g["out"].clone()
            if rows_form:           # the caller zeroes the unmarked rows afterwards
                hip.call("vlr_rows_mask", r.at("out"), r.inp["out"].ld, c.groups * c.N, r.rowmask, c.M)
                torch.cuda.synchronize()
            results.append(r.g["out"].clone())
    finally:
        torch.cuda.synchronize()
        restore(hip)
    first, second = (t.cpu() for t in results)
    assert torch.equal(L.row_bits(first), L.row_bits(second)), f"{c.name}: two runs differ"
    for k, b in r.inp.items():          # the operands are read-only
        if isinstance(b, L.Buf) and k not in ("out", "scratch"):
            assert torch.equal(L.row_bits(r.g[k].cpu()), L.row_bits(b.flat)), f"{c.name}: operand {k} was written"
    if r.rowmask is not None:
        assert torch.equal(r.rowmask.cpu(), r.inp["rowmask"]), f"{c.name}: the row set was written"
    # ---- the routes that have an observable
    if c.kind == "grp":
        assert wrote_ws == (c.splits > 0), f"{c.name}: split-K workspace {'written' if wrote_ws else 'untouched'}, expected {c.splits} slices"
    else:
        assert not wrote_ws, f"{c.name}: the split-K workspace was written"
    if c.kind == "dx" and "walk" in c.name:
        assert cus == (c.comm_cus if c.comm_cus >= 0 else L.COMPUTE_CUS), (c.name, cus)
        assert L.dx_ranges(c, cus) == ([3, 3, 1] if c.comm_cus == 128 else [2, 2, 2, 1]), c.name
    if rows_form and not c.splits:      # 128-row tiles without a marked row are not computed: their rows still hold what they held
        b = r.inp["out"]
        skipped = ~L.slab_marked(r.inp["rowmask"], c.M, 128)
        before, after = L.row_bits(L.logical(b)), L.row_bits(L.logical(b, raw.cpu()))
        assert torch.equal(after[skipped], before[skipped]), f"{c.name}: a tile without a marked row was written"
        assert bool(torch.isnan(L.logical(b)[skipped]).all())
    if r.ktl is not None:
        want = L.tile_list(r.inp["rowmask"], c.K)
        got = r.ktl.cpu()[L.GUARD:].tolist()
        assert got[:len(want)] == want and all(v == L.INT_POISON[torch.int32] for v in got[len(want):]), f"{c.name}: tile list {got}, expected {want}"
    e = L.expect(c, r.inp)
    if e.rel is not None:
        say(f"{c.name}: worst |error| / bound = {L.ratio(c, first, r.inp, e):.3f}")
    L.verify(c, first, r.inp, e)


@pytest.mark.parametrize("name", [c.name for c in L.CASES])
def test_lora_case(hip, name):
    run_case(hip, L.BY_NAME[name])


# ---------------------------------------------------------------------------------------------------- refusals of vlr_lora_rows_u
@pytest.mark.parametrize("what", ["r32", "in96", "n5", "masks-ldx"])
def test_lora_rows_u_refuses(hip, what):
    """a shape outside the contract (r in {64, 128, 256}, in % 64 == 0, n <= 4, packed masks over a dense activation) returns an error and
    leaves u untouched"""
    r, inn, n, ldx, masked = {"r32": (32, 128, 1, 128, 0), "in96": (64, 96, 1, 96, 0), "n5": (64, 128, 5, 128, 0), "masks-ldx": (64, 128, 1, 136, 1)}[what]
    M = 65
    x = torch.ones(M, ldx, dtype=torch.bfloat16, device=DEV)
    A = torch.ones(n * r, inn, dtype=torch.bfloat16, device=DEV)
    u = L.padded(M, n * r, torch.bfloat16, ld=n * r + 8)
    ug = u.flat.to(DEV)
    bits = torch.full((M * inn // 8 + 16,), 0xFF, dtype=torch.uint8, device=DEV) if masked else None
    with pytest.raises((ValueError, hip.VlrError)):
        hip.call("vlr_lora_rows_u", n, x, ldx, A, ug[u.off:], u.ld, r, M, inn, r, 1.0, bits, M * inn // 8 if masked else 0, None)
    torch.cuda.synchronize()
    assert torch.equal(L.row_bits(ug.cpu()), L.row_bits(u.flat)), "u was written by a refused call"


# ---------------------------------------------------------------------------------------------------- helpers
def _exact(name, got, b, ref):
    L.check(name, got.cpu(), b, L.Exp(ref, None, None, None))


@pytest.mark.parametrize("cols", L.BITS2_COLS)
@pytest.mark.parametrize("rows", L.BITS2_ROWS)
def test_dropout_bits2(hip, rows, cols):
    """both packed layouts against the oracle's mask; either output pointer may be null"""
    p, seed = 0.25, 424243 + rows * 1000 + cols
    keep = L.keep_mask(seed, rows, cols, p)
    rm, kt = L.pack_rowmajor(keep), L.pack_kt(keep)
    assert kt.numel() == hip.lib().vlr_dropout_bits_kt_bytes(rows, cols) == L.kt_bytes(rows, cols)
    for want_rm, want_kt in ((1, 1), (1, 0), (0, 1)):
        b1, b2 = L.padded(1, rm.numel(), torch.uint8), L.padded(1, kt.numel(), torch.uint8)
        g1, g2 = b1.flat.to(DEV), b2.flat.to(DEV)
        hip.call("vlr_dropout_bits2", g1[b1.off:] if want_rm else None, g2[b2.off:] if want_kt else None, rows, cols, p, seed)
        torch.cuda.synchronize()
        for want, g, b, ref, nm in ((want_rm, g1, b1, rm, "row-major"), (want_kt, g2, b2, kt, "K-tile-blocked")):
            if want:
                _exact(f"dropout_bits2 {rows} x {cols} {nm}", g, b, ref)
            else:
                assert torch.equal(g.cpu(), b.flat)


@pytest.mark.parametrize("off", [0, 1, 15])
@pytest.mark.parametrize("M", L.TILE_LIST_M)
def test_rows_tile_list(hip, M, off):
    """the marked 64-row tiles, ascending, behind their count; beyond 64 tiles (the second ballot round); a misaligned mask pointer (the
    byte-wise path); marks only in the ragged last tile; entries past 1 + n keep the sentinel"""
    for kind in ("sparse", "dense", "lasttile", "zero"):
        m = L.helper_row_set(M, kind)
        base = torch.full((M + 64,), 1, dtype=torch.uint8, device=DEV)          # marked bytes around the mask: reading past it shows
        base[off:off + M] = m.to(DEV)
        b = L.padded(1, M // 64 + 2, torch.int32)
        g = b.flat.to(DEV)
        hip.call("vlr_rows_tile_list", base[off:], M, g[b.off:])
        torch.cuda.synchronize()
        want = L.tile_list(m, M)
        ref = L.logical(b).clone()
        ref[0, :len(want)] = torch.tensor(want, dtype=torch.int32)
        _exact(f"rows_tile_list M {M} {kind} offset {off}", g, b, ref)


@pytest.mark.parametrize("tile_rows,M", L.TILE_FLAGS)
def test_rows_tile_flags(hip, tile_rows, M):
    for kind in ("sparse", "dense", "lasttile", "zero"):
        m = L.helper_row_set(M, kind, seed=tile_rows)
        base = torch.full((M + 64,), 1, dtype=torch.uint8, device=DEV)
        base[:M] = m.to(DEV)
        b = L.padded(1, -(-M // tile_rows), torch.uint8)
        g = b.flat.to(DEV)
        hip.call("vlr_rows_tile_flags", base, M, tile_rows, g[b.off:])
        torch.cuda.synchronize()
        _exact(f"rows_tile_flags {tile_rows} M {M} {kind}", g, b, L.tile_flags(m, M, tile_rows).view(1, -1))


@pytest.mark.parametrize("cols", L.ROWS_MASK_COLS)
def test_rows_mask(hip, cols):
    """unmarked rows become zero over the first `cols` columns, marked rows and the padding keep their bits"""
    M = 67
    m = L.helper_row_set(M, "dense", seed=cols)
    gen = torch.Generator().manual_seed(cols)
    data = torch.randn(M, cols, generator=gen).to(torch.bfloat16)
    b = L.padded(M, cols, torch.bfloat16, ld=cols + 8, data=data)
    g = b.flat.to(DEV)
    hip.call("vlr_rows_mask", g[b.off:], b.ld, cols, m.to(DEV), M)
    torch.cuda.synchronize()
    _exact(f"rows_mask cols {cols}", g, b, torch.where(m.bool()[:, None], data, torch.zeros_like(data)))


@pytest.mark.parametrize("r1,r2,rows", L.CONCAT)
def test_lora_concat_b(hip, r1, r2, rows):
    gen = torch.Generator().manual_seed(r1 * 7 + r2)
    b1 = torch.randn(rows, r1, generator=gen).to(torch.bfloat16)
    b2 = torch.randn(rows, r2, generator=gen).to(torch.bfloat16)
    o1, o2 = L.operand(b1), L.operand(b2)
    b = L.padded(rows, r1 + r2, torch.bfloat16)
    g = b.flat.to(DEV)
    hip.call("vlr_lora_concat_b", o1.flat.to(DEV)[o1.off:], r1, o2.flat.to(DEV)[o2.off:], r2, g[b.off:], rows)
    torch.cuda.synchronize()
    _exact(f"lora_concat_b {r1} + {r2} x {rows}", g, b, torch.cat([b1, b2], 1))
