"""Reference, case table and checker inputs for the LoRA / PLoRA adapter products: csrc/lora_rows.hip (vlr_lora_rows_u / _v), csrc/lora_dx.hip
(vlr_gemm_dropout_acc_multi / _bits / _rows), the masked and grouped paths of csrc/gemm.hip and csrc/gemm128p.hip (vlr_gemm_grouped[_bits]
with mask_on 1 / 2 / 3, the row-set form, the K-tile-list form) and the helpers they depend on (plain module, no pytest hooks; CPU only).
tests/test_lora_checker_host.py runs the checker on the CPU, tests/test_hip_lora_edges.py runs the same cases on the GPU.  Buffers, the
checker and its conventions are those of tests/row_ref.py.

  CASES            one Case per launch (kind "u", "v", "dx", "dx1", "grp"): shapes, leading dimensions, the dropout probability and seed, the
                   row set, the data regime, the route the launch is meant to take
  make(c)          CPU operands as strided Bufs (leading dimension > logical width wherever the entry point takes one; padding, GUARD cells
                   and every row the contract says is NOT read - skipped slabs, unlisted K tiles, the row behind the last one - hold NaN), the
                   keep masks, their packed forms and the row set; the output pre-filled with NaN, or with data where the call accumulates
  expect(c, inp)   Exp: the float64 formula            emulate(c, inp, fault)   the same in fp32, rounded once to bf16, optionally WRONG
  keep masks       oracle.llava_dpo_oracle.dropout_mask(seed + t, rows * cols, p) - never a kernel's output; pack_rowmajor / pack_kt build the
                   two packed layouts of include/vlr.h from it in numpy (bit e of byte i = element 8 i + e; K-tile-blocked transposed: byte
                   ((row / 64) * cols + col) * 8 + (row % 64) / 8, bit row % 8, padding rows zero)

The two data regimes (as tests/gemm_ref.py).
  exact   integers in [-4, 4] (old C / dx within +-64), p in {0, 0.5}, alpha and scale / (1 - p) powers of two: make() asserts that the sum
          of |terms| per element stays below 2^24, so every partial sum in every order is exact in fp32 and the expected output is the
          float64 formula rounded ONCE to bf16, round to nearest even: the comparison is BITWISE and every route of one product (ring,
          register-staged, row-slab, streaming, tile fallback) must hit the same bits.  make() also asserts that every byte column of every
          packed mask (8 consecutive columns) holds kept AND dropped elements.
  gauss   randn * 0.5, p in {0.05, 0.25} (0 without masks).  ELEMENTWISE |out - ref64| <= 2^-8 |ref| + coef mag; mag = the float64 sum of
          |products| (+ |C_old| / |dx_old|); coef = (K_contracted + splits + n_targets + 6) 2^-23: one ulp per sequential fp32 addition
          (tests/gemm_ref.py derives it; 2^-23 because the guides do not document how the bf16 MFMA rounds its internal adds).
Nothing here is derived from a kernel's output.
"""
import numpy as np
import torch

from oracle import llava_dpo_oracle as O
from tests.row_ref import (Buf, padded, logical, check, check_poison, worst_ratio, Exp, GUARD, U_BF16, INT_POISON,      # noqa: F401 (re-exported)
                           pack_bits, dropout_scale)

F64, F32, BF16, U8 = torch.float64, torch.float32, torch.bfloat16, torch.uint8
U_MFMA = 2.0 ** -23
NAN = float("nan")
COMPUTE_CUS = 256                  # the grid formulas below are written down for the whole chip
LR_MAXT = 8                        # csrc/lora_rows.hip: (pseudo-)targets of one launch; r = 256 counts twice


class Case(dict):
    __getattr__ = dict.__getitem__

    def __repr__(self):
        return self["name"]


def row_bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


# ---------------------------------------------------------------------------------------------------- masks and their layouts
def keep_mask(seed, rows, cols, p):
    """bool [rows][cols]: the keep mask of vlr_dropout(seed) over the dense [rows][cols] operand (index row * cols + col)"""
    if p == 0:
        return torch.ones(rows, cols, dtype=torch.bool)
    return O.dropout_mask(seed, rows * cols, p).view(rows, cols).bool()


def pack_rowmajor(keep):
    """[rows][cols] bool -> uint8 [rows * cols / 8]: bit e of byte i = element 8 i + e of the dense operand (vlr_dropout_bits)"""
    return pack_bits(keep.reshape(-1).to(U8))


def unpack_rowmajor(bits, rows, cols):
    return torch.from_numpy(np.unpackbits(bits.numpy(), bitorder="little")).view(rows, cols).bool()


def kt_bytes(rows, cols):
    return -(-rows // 64) * cols * 8


def pack_kt(keep):
    """[rows][cols] bool -> uint8 [ceil(rows / 64) * cols * 8]: byte ((row / 64) * cols + col) * 8 + (row % 64) / 8, bit row % 8; the rows past
    the last one are zero (vlr_dropout_bits2's second form)"""
    rows, cols = keep.shape
    T = -(-rows // 64)
    m = np.zeros((T * 64, cols), dtype=np.uint8)
    m[:rows] = keep.numpy()
    b = np.packbits(m.reshape(T, 8, 8, cols), axis=2, bitorder="little")          # [tile][byte of the tile][1][col]
    return torch.from_numpy(np.ascontiguousarray(b.reshape(T, 8, cols).transpose(0, 2, 1)).reshape(-1))


def unpack_kt(bits, rows, cols):
    T = -(-rows // 64)
    b = bits.numpy().reshape(T, cols, 8).transpose(0, 2, 1)                        # [tile][byte][col]
    m = np.unpackbits(np.ascontiguousarray(b).reshape(T, 8, 1, cols), axis=2, bitorder="little")
    return torch.from_numpy(m.reshape(T * 64, cols)[:rows].copy()).bool()


def kt_byte_of(row, col, cols):
    """(byte index, bit) of element (row, col) in the K-tile-blocked transposed layout - the formula of include/vlr.h, one element at a time"""
    return ((row // 64) * cols + col) * 8 + (row % 64) // 8, row % 8


def row_set(kind, M, slab):
    """uint8 [M] (1 = the row takes part) or None.  slab = the rows one workgroup / tile owns.
    zero: no row; last: only the last valid row; row0: only row 0 of one slab (the second when there is one); gap: an unmarked slab between
    two marked ones; ragged: a run that starts and ends inside slabs plus marks in the ragged last slab; lasttile: only the last row, which
    sits in a ragged last slab"""
    if kind is None:
        return None
    m = torch.zeros(M, dtype=U8)
    ns = -(-M // slab)
    if kind == "last" or kind == "lasttile":
        m[M - 1] = 1
    elif kind == "row0":
        m[min(1, ns - 1) * slab] = 1
    elif kind == "gap":
        assert ns >= 3
        m[3:slab - 5:7] = 1
        m[2 * slab + 1] = 1
        m[min(M, 3 * slab) - 1] = 1
    elif kind == "ragged":
        assert ns >= 2 and M % slab
        m[slab // 2:slab + 9] = 1
        m[(ns - 1) * slab:M:3] = 1
    else:
        assert kind == "zero", kind
    return m


def slab_marked(mask, M, slab):
    """bool [M]: the row's slab holds a marked row"""
    ns = -(-M // slab)
    pad = torch.zeros(ns * slab, dtype=torch.bool)
    pad[:M] = mask.bool()
    return pad.view(ns, slab).any(1).repeat_interleave(slab)[:M]


def tile_list(mask, M):
    """what vlr_rows_tile_list writes: [n, the 64-row tiles with a marked row ...]"""
    ns = -(-M // 64)
    pad = torch.zeros(ns * 64, dtype=torch.bool)
    pad[:M] = mask.bool()
    t = pad.view(ns, 64).any(1).nonzero().flatten().tolist()
    return [len(t)] + t


def tile_flags(mask, M, tile_rows):
    """what vlr_rows_tile_flags writes: 1 = NO marked row in the tile"""
    ns = -(-M // tile_rows)
    pad = torch.zeros(ns * tile_rows, dtype=torch.bool)
    pad[:M] = mask.bool()
    return (~pad.view(ns, tile_rows).any(1)).to(U8)


# ---------------------------------------------------------------------------------------------------- the launchers' routes (256 compute CUs)
def u_slab(c):
    """rows one workgroup of lora_rows_kernel owns (vlr_lora_rows_try_launch: r = 256 runs 128-row workgroups)"""
    return 128 if c.r == 256 else 64


def dx_streams(c):
    """vlr_lora_dx_try_launch takes the shape (else dropacc_multi_kernel, the 128 x 128 tile fallback)"""
    return 1 <= c.n <= 3 and c.inn % 128 == 0 and c.r in (64, 128, 256) and not (c.r == 256 and c.n > 2)


def dx_slab(c):
    """rows one workgroup of lora_dx_kernel owns: 128 where the v fragments fit 8 waves' registers AND (r = 256 or in >= 8192)"""
    kt = c.r // 64
    return 128 if c.n * kt <= 4 and (kt == 4 or c.inn >= 8192) else 64


def dx_ranges(c, cus=COMPUTE_CUS):
    """column tiles per blockIdx.y of the streaming kernel (vlr_lora_dx_try_launch's grid formula)"""
    rows = dx_slab(c)
    rb, tiles_n = -(-c.M // rows), c.inn // 128
    wpc = 2 if rows == 128 and c.inn < 8192 else 4
    splits = max(1, min(tiles_n, -(-wpc * cus // rb)))
    ct = -(-tiles_n // splits)
    return [min(ct, tiles_n - i) for i in range(0, tiles_n, ct)]


def grp_splits(c):
    """split-K slices of gemm_grouped (0: un-split), given the 64 MiB slot the test registers"""
    tiles = -(-c.Mo // 128) * -(-c.No // 128)
    if not (tiles * c.groups < 384 and c.K >= 1024):
        return 0
    s = min(512 // (tiles * c.groups), 16, c.K // 256)
    if s < 2:
        return 0
    kchunk = -(-(-(-c.K // s)) // 64) * 64
    return -(-c.K // kchunk)


# ---------------------------------------------------------------------------------------------------- the case table
def _seed(*k):
    s = 7
    for v in k:
        s = (s * 1000003 + int(v)) % 2147483647
    return s


def _base(kind, name, regime, masked, **kw):
    p = kw.pop("p", None)
    if p is None:
        p = (0.5 if regime == "exact" else 0.25) if masked else 0.0
    c = Case(kind=kind, name=name, regime=regime, masked=masked, p=p, rowmask=None, comm_cus=-1, acc=0, **kw)
    return c


def _u(r, steps, M, n, masked, regime="exact", tag="", ustride=0, ldx_pad=0, rowmask=None, p=None, alpha=None):
    inn = 64 * steps
    us = ustride or r
    name = f"u-r{r}-k{steps}-M{M}-n{n}-{'bits' if masked else 'nomask'}-{regime}" + (f"-{tag}" if tag else "")
    c = _base("u", name, regime, masked, p=p, r=r, inn=inn, M=M, n=n, ustride=us, ldx=inn + ldx_pad, ldu=(n - 1) * us + r + 8, Kc=inn,
              alpha=alpha if alpha is not None else (0.5 if regime == "exact" else 0.25), seed=_seed(1, r, steps, M, n))
    c["rowmask"] = rowmask
    return c


def _v(r, outs, M, regime="exact", tag="", rowmask=None):
    n = len(outs)
    name = f"v-r{r}-o{'.'.join(map(str, outs))}-M{M}-{regime}" + (f"-{tag}" if tag else "")
    c = _base("v", name, regime, False, r=r, outs=tuple(outs), inn=max(outs), M=M, n=n, lddy=sum(outs) + 8, ldv=n * r + 8, Kc=max(outs), alpha=1.0,
              seed=_seed(2, r, M, *outs))
    c["rowmask"] = rowmask
    return c


def _dx(n, r, inn, M, mode, acc, regime="exact", tag="", rowmask=None, entry=None, comm_cus=-1, nan_rows=True, p=None, scale=None):
    """mode: "p0" (no dropout), "hash" (p > 0, bits NULL: the kernel hashes), "bits" (packed masks)"""
    masked = mode != "p0"
    entry = entry or ("rows" if rowmask else "bits" if mode == "bits" else "multi")
    name = f"dx-n{n}-r{r}-in{inn}-M{M}-{mode}-acc{acc}-{regime}" + (f"-{tag}" if tag else "")
    c = _base("dx", name, regime, masked, p=p, n=n, r=r, inn=inn, M=M, mode=mode, entry=entry, ldv=n * r + 8, Kc=r, seed=_seed(3, n, r, inn, M, acc),
              scale=scale if scale is not None else ((1.0 if masked else 0.5) if regime == "exact" else 0.25))      # scale / (1 - p) = 2 or 0.5
    c.update(acc=acc, rowmask=rowmask, comm_cus=comm_cus, nan_rows=nan_rows)
    return c


def _dx1(r, inn, M, mode, regime="exact", tag="", misalign=None):
    """vlr_gemm_dropout_acc / _bits (one target, always +=): the masked epilogue of the register-staged 128 x 128 kernel.  misalign "v" /
    "dx": that operand starts 8 bytes off a 16-byte boundary, which sends the call to product -> scratch, vlr_dropout(add) -> dx.  That
    path rounds twice, so its cases have r = 16: |v . A| <= 256 is exact in bf16 and the second rounding is the only one.  (The third
    path of the entry point, the 256 x 256 kernel's epilogue, is tried only for operands that are NOT 16-byte aligned and itself requires
    them aligned: no shape reaches it.)"""
    assert not misalign or (r == 16 and regime == "exact")
    name = f"dx1-r{r}-in{inn}-M{M}-{mode}-{regime}" + (f"-{tag}" if tag else "")
    c = _base("dx1", name, regime, mode != "p0", n=1, r=r, inn=inn, M=M, mode=mode, entry="one", ldv=r + 8, Kc=r, seed=_seed(4, r, inn, M),
              scale=((1.0 if mode != "p0" else 0.5) if regime == "exact" else 0.25), misalign=misalign, nan_rows=False)
    c["acc"] = 1
    return c


def _g(mask_on, M, K, groups, mode, acc=0, regime="exact", tag="", N=None, r=64, rowmask=None, ktl=None, layout=None, entry=None):
    """vlr_gemm_grouped[_bits / _bits_rows / _bits_ktiles].
    mask_on 1 (NT): C [M][g N .. + N] = alpha (keep_g . x [M][K]) A_g [N][K]^T - x dense and shared, N = r.
    mask_on 2 / 3 (TN): C_g [r][in] = alpha v_g [K][r]^T (keep_g . x [K][in]) - K = token rows, v the groups side by side, x dense and shared.
    mask_on 0: layout 0 / 1: C [M][g N ..] = alpha x_g W_g (the row-set form); layout 2: dB_g [out][r] = dy_g [K][out]^T u_g [K][r] (the
    K-tile-list form).  mode "hash" / "bits" / "p0"."""
    layout = layout if layout is not None else (0 if mask_on == 1 else 2)
    masked = mask_on != 0
    entry = entry or ("ktiles" if ktl is not None else "rows" if rowmask else "bits" if mode == "bits" else "grouped")
    if layout == 2:
        inn = N or 128
        name = f"grp-tn-mask{mask_on}-K{K}-in{inn}-r{r}-g{groups}-{mode}-acc{acc}-{regime}"
        c = _base("grp", name, regime, masked, layout=2, mask_on=mask_on, M=K, K=K, inn=inn, r=r, N=inn, groups=groups, mode=mode, entry=entry,
                  Kc=K, alpha=0.5 if regime == "exact" else 0.25, seed=_seed(5, mask_on, K, inn, groups, acc))
    else:
        N = N or r
        name = f"grp-{'nt' if layout == 0 else 'nn'}-mask{mask_on}-M{M}-K{K}-N{N}-g{groups}-{mode}-acc{acc}-{regime}"
        c = _base("grp", name, regime, masked, layout=layout, mask_on=mask_on, M=M, K=K, N=N, inn=K, r=N, groups=groups, mode=mode, entry=entry,
                  Kc=K, alpha=0.5 if regime == "exact" else 0.25, seed=_seed(6, mask_on, M, K, N, groups, acc))
    c["name"] += f"-{tag}" if tag else ""
    c.update(acc=acc, rowmask=rowmask, ktl=ktl)
    c["Mo"], c["No"] = ((c.r, c.inn) if mask_on else (c.inn, c.r)) if layout == 2 else (c.M, c.N)      # one group's output
    c["splits"] = grp_splits(c)
    return c


ROWSETS = ("zero", "last", "row0", "gap", "ragged")


def _build_cases():
    cs = []
    # ---- vlr_lora_rows_u: K steps against the ring depth (6 stages at r 64 / 128: 5 steps in flight; 4 stages at r 256), slab raggedness,
    # more than 8 slabs (the slab <-> XCD map wraps), n * parts up to LR_MAXT, with and without packed masks
    for r in (64, 128):
        for steps, M, n, mk in ((1, 1, 1, 0), (2, 63, 3, 1), (4, 64, 4, 0), (5, 65, 1, 1), (6, 129, 3, 0), (7, 513, 4, 1), (13, 577, 1, 1),
                                (1, 129, 4, 1), (6, 64, 2, 1), (13, 65, 3, 0)):
            cs.append(_u(r, steps, M, n, mk))
        cs += [_u(r, 2, 65, 3, 1, tag="ustride", ustride=r + 16), _u(r, 4, 129, 2, 0, tag="ldx", ldx_pad=72),
               _u(r, 13, 577, 3, 1, "gauss", p=0.05), _u(r, 5, 65, 4, 1, "gauss", p=0.25, ustride=r + 8, tag="ustride"), _u(r, 7, 129, 1, 0, "gauss")]
        for rs in ROWSETS:
            cs.append(_u(r, 2, 193, 2, 1, tag=f"rows-{rs}", rowmask=rs))
        cs.append(_u(r, 6, 193, 1, 0, "gauss", tag="rows-gap", rowmask="gap"))
    for steps, M, n, mk in ((1, 1, 1, 0), (2, 63, 3, 1), (3, 64, 4, 0), (4, 65, 1, 1), (5, 129, 4, 1), (9, 513, 3, 0), (2, 577, 1, 1), (3, 1025, 1, 1),
                            (4, 128, 2, 1), (9, 129, 1, 0)):
        cs.append(_u(256, steps, M, n, mk))
    cs += [_u(256, 2, 65, 3, 1, tag="ustride", ustride=256 + 16), _u(256, 4, 129, 2, 0, tag="ldx", ldx_pad=72),
           _u(256, 9, 577, 3, 1, "gauss", p=0.05), _u(256, 5, 65, 4, 1, "gauss", p=0.25), _u(256, 3, 129, 1, 0, "gauss")]
    for rs in ROWSETS:
        cs.append(_u(256, 2, 385, 2, 1, tag=f"rows-{rs}", rowmask=rs))
    # ---- vlr_lora_rows_v: unequal outs per target (the targets walk different step counts inside one launch), lddy > sum(outs)
    for r, big in ((64, 0), (128, 0), (256, 1)):
        M9 = 1025 if big else 513
        for outs, M in (((64,), 1), ((64, 192, 128), 63), ((320, 64), 64), ((128, 128, 64, 384), 65), ((448,), 129), ((64, 192, 128), M9),
                        ((832, 64), 577)):
            cs.append(_v(r, outs, M))
        cs += [_v(r, (64, 192, 128), 577, "gauss"), _v(r, (320, 64), 65, "gauss")]
        Mr = 385 if big else 193
        for rs in ROWSETS:
            cs.append(_v(r, (128, 64), Mr, tag=f"rows-{rs}", rowmask=rs))
    # ---- vlr_gemm_dropout_acc_multi / _bits / _rows: every template the launcher reaches
    ms = (1, 63, 65, 129)
    k = 0
    for n, r in ((1, 64), (2, 64), (3, 64), (1, 128), (2, 128), (3, 128), (2, 256)):            # the 64-row form
        for mode in ("p0", "hash", "bits"):
            for acc in (0, 1):
                cs.append(_dx(n, r, 128 if (k % 2) else 256, ms[k % 4], mode, acc))
                k += 1
        cs.append(_dx(n, r, 384, 129, "bits", 1, "gauss", p=0.05))
    for inn in (128, 256):                                                                      # the 128-row form: n = 1, r = 256
        for mode, acc, M in (("p0", 0, 1), ("hash", 1, 129), ("bits", 0, 65), ("bits", 1, 257)):
            cs.append(_dx(1, 256, inn, M, mode, acc))
    cs.append(_dx(1, 256, 256, 129, "hash", 1, "gauss", p=0.25))
    # the 128-row form: in = 8192.  (One row has 8 elements per byte column and 1024 byte columns: no seed gives an all-mixed mask, so the
    # masked M = 1 case is a gauss one and the exact M = 1 case runs without dropout.)
    for n, r in ((1, 64), (3, 64), (2, 128)):
        cs += [_dx(n, r, 8192, 1, "p0", 0), _dx(n, r, 8192, 1, "bits", 1, "gauss", p=0.25), _dx(n, r, 8192, 129, "bits", 1),
               _dx(n, r, 8192, 129, "hash", 0, "gauss", p=0.05)]
    # the column-range walk: 172 row blocks of 64, 7 column tiles -> workgroups own 2, 2, 2, 1 (3, 3, 1 with 128 CUs left to compute)
    cs += [_dx(2, 64, 896, 10945, "bits", 1, tag="walk"), _dx(3, 64, 896, 10945, "bits", 0, tag="walk"),
           _dx(2, 64, 896, 10945, "bits", 1, tag="walk-comm128", comm_cus=128), _dx(2, 64, 896, 10945, "hash", 1, "gauss", tag="walk", p=0.25)]
    # the row set: accumulate = 1 skips the slabs without a marked row (their v rows are NaN here), accumulate = 0 writes every row
    for n, r, inn, M in ((2, 64, 256, 193), (1, 256, 128, 385)):
        for rs in ROWSETS:
            cs.append(_dx(n, r, inn, M, "bits", 1, tag=f"rows-{rs}", rowmask=rs))
        cs += [_dx(n, r, inn, M, "bits", 0, tag="rows-gap", rowmask="gap"), _dx(n, r, inn, M, "p0", 0, tag="rows-zero", rowmask="zero")]
    cs.append(_dx(2, 128, 8192, 385, "bits", 1, tag="rows-gap", rowmask="gap"))
    # the fallback tile kernel
    for n, r, inn in ((2, 16, 128), (2, 64, 136), (5, 64, 128), (3, 256, 128)):
        cs += [_dx(n, r, inn, 129, "bits", 1, tag="tile"), _dx(n, r, inn, 65, "hash", 0, tag="tile")]
    cs += [_dx(5, 64, 128, 129, "bits", 1, "gauss", tag="tile", p=0.05), _dx(2, 64, 136, 385, "bits", 1, tag="tile-rows-gap", rowmask="gap", nan_rows=False)]
    # the single-target call (the 128 x 128 kernel's masked epilogue)
    cs += [_dx1(64, 256, 129, "bits"), _dx1(128, 136, 65, "hash"), _dx1(64, 128, 63, "p0"), _dx1(64, 256, 129, "bits", "gauss"),
           _dx1(16, 136, 129, "hash", tag="v+8B", misalign="v"), _dx1(16, 256, 65, "bits", tag="dx+8B", misalign="dx")]
    # ---- vlr_gemm_grouped / _bits with masks.  NT (mask_on 1): K = 72 hashes even when bits are passed; 1024 / 1088 are split along K
    k = 0
    for K in (64, 72, 128, 1024, 1088):
        for groups, M in ((1, 127), (3, 1), (8, 129)):
            cs.append(_g(1, M, K, groups, "bits" if k % 3 else "hash", acc=k % 2))
            k += 1
    cs += [_g(1, 129, 1088, 3, "bits", 1, "gauss"), _g(1, 127, 72, 3, "bits", 0, "gauss"), _g(1, 129, 128, 8, "hash", 0, "gauss")]
    # TN (mask_on 2 hashes / reads row-major bits, mask_on 3 reads the K-tile-blocked bits; in = 136 sends 3 to the hashing fallback)
    for K in (8, 63, 64, 65, 130, 1024, 1100):
        for inn in (128, 136):
            acc = (K + inn // 8) % 2
            cs += [_g(2, 0, K, 3, "hash", acc, N=inn), _g(2, 0, K, 2, "bits", 1 - acc, N=inn), _g(3, 0, K, 3, "bits", acc, N=inn)]
    cs += [_g(3, 0, 1100, 3, "bits", 1, "gauss", N=128), _g(3, 0, 130, 2, "bits", 0, "gauss", N=136), _g(2, 0, 1100, 3, "hash", 1, "gauss", N=128)]
    # ---- vlr_gemm_grouped_bits_rows (layouts 0 / 1, accumulate 0): tiles of 128 rows without a marked row are not computed
    for rs in ("gap", "ragged", "lasttile", "zero"):
        cs += [_g(1, 385, 128, 2, "bits", 0, tag=f"rows-{rs}", rowmask=rs), _g(0, 385, 128, 2, "p0", 0, tag=f"rows-{rs}", rowmask=rs, layout=1, N=64)]
    cs.append(_g(1, 385, 128, 2, "bits", 0, "gauss", tag="rows-gap", rowmask="gap"))
    # ---- vlr_gemm_grouped_bits_ktiles (layout 2): dB = dy^T u unmasked, dA = v^T (keep . x) with mask_on 3
    for kt in ("first", "last", "all", "empty", "gap"):
        for acc in (0, 1):
            cs += [_g(0, 0, 320, 2, "p0", acc, tag=f"kt-{kt}", ktl=kt, N=128), _g(3, 0, 320, 2, "bits", acc, tag=f"kt-{kt}", ktl=kt, N=128)]
    cs += [_g(0, 0, 328, 2, "p0", 1, tag="kt-ignored", ktl="gap", N=128), _g(3, 0, 328, 2, "bits", 0, tag="kt-ignored", ktl="gap", N=128),
           _g(3, 0, 1280, 2, "bits", 1, tag="kt-gap", ktl="gap", N=128), _g(3, 0, 320, 2, "bits", 1, "gauss", tag="kt-gap", ktl="gap", N=128),
           _g(0, 0, 1280, 2, "p0", 0, "gauss", tag="kt-all", ktl="all", N=128)]
    names = [c.name for c in cs]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return cs


def kt_row_set(c):
    """the row set behind a K-tile list: uint8 [K]"""
    K, nt = c.K, -(-c.K // 64)
    m = torch.zeros(K, dtype=U8)
    if c.ktl == "first":
        m[5] = 1
    elif c.ktl == "last":
        m[(K // 64 - 1) * 64 + 63] = 1            # the last whole tile
    elif c.ktl == "all":
        m[::64] = 1
        m[K - 1] = 1
    elif c.ktl == "gap":
        for t in range(0, nt, 2):
            m[t * 64 + (7 * t) % 64] = 1
    else:
        assert c.ktl == "empty"
    return m


CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}
FAMILY = {"u": "vlr_lora_rows_u", "v": "vlr_lora_rows_v", "dx": "vlr_gemm_dropout_acc_multi[_bits/_rows]", "dx1": "vlr_gemm_dropout_acc[_bits]",
          "grp": "vlr_gemm_grouped[_bits]"}


def family(c):
    if c.kind == "grp" and c.entry in ("rows", "ktiles"):
        return "vlr_gemm_grouped_bits_" + c.entry
    return FAMILY[c.kind]


# ---------------------------------------------------------------------------------------------------- operands
def _values(c, shape, g, lim=4):
    if c.regime == "gauss":
        return (torch.randn(*shape, generator=g) * 0.5).to(BF16)
    return torch.randint(-lim, lim + 1, shape, generator=g).to(BF16)


def operand(data, ld=None, extra=1):
    """a read-only operand: its rows behind GUARD cells of NaN, NaN in the padding of every row and `extra` rows of NaN behind the last"""
    rows, width = data.shape
    b = padded(rows + extra, width, data.dtype, ld=ld)
    b = Buf(b.flat, b.off, rows, width, b.ld)
    logical(b)[:] = data
    return b


def _bits_buf(keeps, packer, align=16):
    """the packed masks of the targets behind GUARD bytes, target t at t * gstride (sentinel bytes between them) -> (Buf, gstride)"""
    packed = [packer(k) for k in keeps]
    nb = packed[0].numel()
    gs = -(-nb // align) * align + align
    b = padded(1, gs * len(packed), U8)
    for t, pk in enumerate(packed):
        logical(b)[0, t * gs:t * gs + nb] = pk
    return b, gs


def mixed(keep, rows_used=None):
    """every byte column (8 consecutive columns) of the mask holds kept and dropped elements among the rows the case reads"""
    k = keep if rows_used is None else keep[rows_used]
    if k.shape[0] == 0:
        return True
    g = k.reshape(k.shape[0], -1, 8)
    return bool((g.any(2).any(0) & (~g).any(2).any(0)).all())


def _keeps(c, n, rows, cols, rows_used=None):
    """(seed, the n keep masks of vlr_dropout(seed + t) over [rows][cols]); exact regime: the first of c.seed, c.seed + 1009, ... whose
    masks are all mixed (a one-row case has 8 elements per byte column: now and then they agree)"""
    if not c.masked:
        return c.seed, None
    for bump in range(256):
        seed = c.seed + 1009 * bump
        keep = [keep_mask(seed + t, rows, cols, c.p) for t in range(n)]
        if c.regime != "exact" or all(mixed(k, rows_used) for k in keep):
            return seed, keep
    raise AssertionError(f"{c.name}: no seed with mixed masks")


def _finish(c, inp, top):
    if c.regime == "exact":
        assert top < 2 ** 24, (c.name, top)                 # the sum of |terms| per element: every fp32 partial sum in every order is exact
        if c.masked:
            assert c.p == 0.5
            for k in inp["keep"]:
                assert mixed(k, inp.get("rows_used")), f"{c.name}: a byte column of the keep mask is all kept or all dropped"
    else:
        assert c.p in (0.0, 0.05, 0.25)
    return inp


def _pow2(x):
    return x > 0 and float(np.log2(x)).is_integer()


def make(c):
    g = torch.Generator().manual_seed(c.seed)
    return {"u": _make_u, "v": _make_v, "dx": _make_dx, "dx1": _make_dx, "grp": _make_grp}[c.kind](c, g)


def _make_u(c, g):
    M, inn, r, n = c.M, c.inn, c.r, c.n
    x = _values(c, (M, inn), g)
    rm = row_set(c.rowmask, M, u_slab(c))
    if rm is not None:
        x[~slab_marked(rm, M, u_slab(c))] = NAN            # a slab without a marked row is not read
    A = _values(c, (n * r, inn), g)
    rows_used = None if rm is None else slab_marked(rm, M, u_slab(c))
    seed, keep = _keeps(c, n, M, inn, rows_used)
    inp = dict(x=operand(x, c.ldx), A=operand(A), out=padded(M, (n - 1) * c.ustride + r, BF16, ld=c.ldu), rowmask=rm, keep=keep, seed=seed,
               rows_used=rows_used)
    if c.masked:
        inp["bits"], inp["gstride"] = _bits_buf(keep, pack_rowmajor)
    if c.regime == "exact":
        assert _pow2(c.alpha)
    return _finish(c, inp, 16 * inn * c.alpha)


def _make_v(c, g):
    M, r, n = c.M, c.r, c.n
    dy = _values(c, (M, sum(c.outs)), g)
    rm = row_set(c.rowmask, M, u_slab(c))
    if rm is not None:
        dy[~slab_marked(rm, M, u_slab(c))] = NAN
    B = _values(c, (sum(c.outs), r), g)
    inp = dict(x=operand(dy, c.lddy), A=operand(B), out=padded(M, n * r, BF16, ld=c.ldv), rowmask=rm, keep=None)
    return _finish(c, inp, 16 * max(c.outs))


def _make_dx(c, g):
    M, inn, r, n = c.M, c.inn, c.r, c.n
    v = _values(c, (M, n * r), g)
    rm = row_set(c.rowmask, M, dx_slab(c) if dx_streams(c) else 128)
    if rm is not None:
        v[rm == 0] = 0                                      # the caller's guarantee: zero v rows on the unmarked rows
        if c.acc and c.nan_rows:
            assert dx_streams(c)
            v[~slab_marked(rm, M, dx_slab(c))] = NAN        # ... and with accumulate = 1 a slab without a marked row is not read
    A = _values(c, (n * r, inn), g)
    d0 = _values(c, (M, inn), g, 64) if c.acc else None
    seed, keep = _keeps(c, n, M, inn)
    inp = dict(x=operand(v, c.ldv), A=operand(A), out=padded(M, inn, BF16, data=d0), rowmask=rm, keep=keep, seed=seed)
    if c.mode == "bits":
        inp["bits"], inp["gstride"] = _bits_buf(keep, pack_rowmajor)
    if c.kind == "dx1":
        inp["scratch"] = padded(M, inn, BF16)
        if c.misalign:
            k = "x" if c.misalign == "v" else "out"
            b = inp[k]
            inp[k] = Buf(torch.cat([torch.full((4,), NAN, dtype=BF16), b.flat]), b.off + 4, b.rows, b.width, b.ld)
    if c.regime == "exact":
        assert _pow2(dropout_scale(c.p, c.scale))
    return _finish(c, inp, 16 * r * n * dropout_scale(c.p, c.scale) + 64)


def _make_grp(c, g):
    ng, K = c.groups, c.K
    rm = None
    if c.layout == 2:                                       # C_g [Mo][No] = alpha a_g [K][Mo]^T b_g [K][No]; b = x [K][in] shared when masked
        Mo, No = (c.r, c.inn) if c.mask_on else (c.inn, c.r)
        a = _values(c, (K, ng * Mo), g)
        b = _values(c, (K, No if c.mask_on else ng * No), g)
        if c.ktl is not None:
            rm = kt_row_set(c)
            a[rm == 0] = 0                                  # the caller's guarantee: every unmarked row contributes zero
            if K % 64 == 0:
                listed = slab_marked(rm, K, 64)
                a[~listed] = NAN                            # the unlisted K tiles of both operands are not read
                b[~listed] = NAN
        A, B = operand(a, ng * Mo + 8), operand(b, None if c.mask_on else ng * No + 8)
        c0 = _values(c, (ng * Mo, No), g, 64) if c.acc else None
        out = padded(ng * Mo, No, BF16, ld=No + 8, data=c0)
        rows_used = None if rm is None or K % 64 else slab_marked(rm, K, 64)
        seed, keep = _keeps(c, ng, K, No, rows_used)
    else:                                                   # C [M][g N .. + N] = alpha a_g b_g: NT a = x [M][K] shared (masked) / b_g [N][K];
        M, N = c.M, c.N                                     # NN a_g = x [M][g K .. + K] / b_g [K][N]
        rm = row_set(c.rowmask, M, 128)
        a = _values(c, (M, K if c.layout == 0 else ng * K), g)
        if rm is not None:
            a[~slab_marked(rm, M, 128)] = NAN               # the skipped tiles' operand rows
        b = _values(c, (ng * N, K) if c.layout == 0 else (ng * K, N), g)
        A = operand(a, None if c.mask_on else a.shape[1] + 8)
        B = operand(b, b.shape[1] + 8)
        c0 = _values(c, (M, ng * N), g, 64) if c.acc else None
        out = padded(M, ng * N, BF16, ld=ng * N + 8, data=c0)
        rows_used = None if rm is None else slab_marked(rm, M, 128)
        seed, keep = _keeps(c, ng, M, K, rows_used)
    inp = dict(x=A, A=B, out=out, rowmask=rm, keep=keep, rows_used=rows_used, seed=seed)
    if c.mode == "bits":
        inp["bits"], inp["gstride"] = _bits_buf(keep, pack_kt if c.mask_on == 3 else pack_rowmajor)
    if c.regime == "exact":
        assert _pow2(c.alpha)
    return _finish(c, inp, 16 * K * c.alpha + 64)


# ---------------------------------------------------------------------------------------------------- the formulas
def out_cols(c):
    """the logical columns of the output buffer the call writes (None: all of them)"""
    if c.kind == "u" and c.ustride != c.r:
        return torch.cat([torch.arange(t * c.ustride, t * c.ustride + c.r) for t in range(c.n)])
    return None


def _rows_on(x, rm):
    """the operand with its unmarked rows (NaN in skipped slabs) replaced by zero"""
    if rm is None:
        return x
    return torch.where(rm.bool()[:, None], torch.nan_to_num(x), torch.zeros_like(x))


def formula(c, inp, dt, fault=None):
    """(value, sum of |terms|) of the written columns in dtype dt.  fault (the host test's planted errors): ("flip", t, row, col) one keep
    bit flipped; "lastk" the last K step of 64 dropped; "alpha2" alpha applied twice"""
    x, W, rm = logical(inp["x"]).to(dt), logical(inp["A"]).to(dt), inp["rowmask"]
    keep = None if inp["keep"] is None else [k.clone() for k in inp["keep"]]
    if isinstance(fault, tuple):
        _, t, i, j = fault
        keep[t][i, j] = ~keep[t][i, j]
    kf = (lambda t: keep[t].to(dt)) if keep is not None else (lambda t: 1.0)
    cut = 64 if fault == "lastk" else 0
    vals, mags = [], []
    if c.kind == "u":
        xe = _rows_on(x, rm)
        a = c.alpha * (c.alpha if fault == "alpha2" else 1.0)
        for t in range(c.n):
            xm, At = (xe * kf(t))[:, :c.inn - cut], W[t * c.r:(t + 1) * c.r, :c.inn - cut]
            vals.append(a * (xm @ At.t()))
            mags.append(a * (xm.abs() @ At.abs().t()))
    elif c.kind == "v":
        xe, ofs = _rows_on(x, rm), 0
        for t, o in enumerate(c.outs):
            oc = o - (cut if t == c.n - 1 else 0)
            vals.append(xe[:, ofs:ofs + oc] @ W[ofs:ofs + oc])
            mags.append(xe[:, ofs:ofs + oc].abs() @ W[ofs:ofs + oc].abs())
            ofs += o
    elif c.kind in ("dx", "dx1"):
        a = dropout_scale(c.p, c.scale) * (dropout_scale(c.p, c.scale) if fault == "alpha2" else 1.0)
        xe = torch.nan_to_num(x) if rm is not None else x              # v is zero on the unmarked rows; NaN only where the slab is skipped
        rc = c.r - cut
        val = sum(kf(t) * (xe[:, t * c.r:t * c.r + rc] @ W[t * c.r:t * c.r + rc]) for t in range(c.n)) * a
        mag = sum(kf(t) * (xe[:, t * c.r:t * c.r + rc].abs() @ W[t * c.r:t * c.r + rc].abs()) for t in range(c.n)) * a
        vals, mags = [val], [mag]
    else:
        a = c.alpha * (c.alpha if fault == "alpha2" else 1.0)
        K = c.K - cut
        if c.layout == 2:
            Mo, No = (c.r, c.inn) if c.mask_on else (c.inn, c.r)
            if c.ktl is not None and c.K % 64 == 0:                     # only the listed K tiles are contracted
                on = slab_marked(inp["rowmask"], c.K, 64)
                x, W = torch.where(on[:, None], x, torch.zeros_like(x)), torch.where(on[:, None], W, torch.zeros_like(W))
            for t in range(c.groups):
                at = x[:K, t * Mo:(t + 1) * Mo]
                bt = (W * kf(t))[:K] if c.mask_on else W[:K, t * No:(t + 1) * No]
                vals.append(a * (at.t() @ bt))
                mags.append(a * (at.abs().t() @ bt.abs()))
            vals, mags = [torch.cat(vals, 0)], [torch.cat(mags, 0)]
        else:
            xe = _rows_on(x, rm)
            for t in range(c.groups):
                if c.layout == 0:
                    at, bt = (xe * kf(t))[:, :K], W[t * c.N:(t + 1) * c.N, :K].t()
                else:
                    at, bt = xe[:, t * c.K:t * c.K + K], W[t * c.K:t * c.K + K]
                vals.append(a * (at @ bt))
                mags.append(a * (at.abs() @ bt.abs()))
    val, mag = torch.cat(vals, 1), torch.cat(mags, 1)
    if c.acc:
        old = logical(inp["out"]).to(dt)
        val, mag = val + old, mag + old.abs()
    return val, mag


def n_targets(c):
    return c.n if c.kind in ("u", "v", "dx", "dx1") else 1


def coef(c):
    return (c.Kc + c.get("splits", 0) + n_targets(c) + 6) * U_MFMA


def expect(c, inp):
    val, mag = formula(c, inp, F64)
    if c.regime == "gauss":
        return Exp(val, mag, U_BF16, coef(c))
    return Exp(val.to(F32), None, None, None)      # an integer multiple of 1/4 below 2^24: exact in fp32, rounded once to bf16 by the comparison


def emulate(c, inp, fault=None, unrounded=False):
    val, _ = formula(c, inp, F32, fault)
    return val if unrounded else val.to(BF16)


def place(c, inp, out, cols=None):
    """the output's flat buffer after a call that wrote `out` into the written columns (cols: other columns, a planted fault)"""
    b = inp["out"]
    f = b.flat.clone()
    cols = out_cols(c) if cols is None else cols
    if cols is None:
        logical(b, f)[:] = out.to(f.dtype)
    else:
        logical(b, f)[:, cols] = out.to(f.dtype)
    return f


def _compact(c, after, b, cols):
    cb = padded(b.rows, len(cols), after.dtype, ld=len(cols) + 8)
    f = cb.flat.clone()
    logical(cb, f)[:] = logical(b, after)[:, cols]
    return cb, f


def verify(c, after, inp, e):
    """the checker: the written columns against e (bitwise / elementwise bound), every other cell of the flat buffer - the columns between
    the targets' blocks, the padding, the guards - bit-identical to what it held before the call"""
    b, cols = inp["out"], out_cols(c)
    if cols is None:
        check(c.name, after, b, e)
        return
    cb, f = _compact(c, after, b, cols)
    check(c.name, f, cb, e)
    keepout = torch.ones(b.flat.numel(), dtype=torch.bool)
    logical(b, keepout)[:, cols] = False
    bad = keepout & (row_bits(after) != row_bits(b.flat))
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{c.name}: cell {i - b.off} of the buffer (outside the targets' blocks, ld {b.ld}) was overwritten ({int(bad.sum())} such cells)")


def ratio(c, after, inp, e):
    """worst |error| / bound of a gauss case (measuring only)"""
    b, cols = inp["out"], out_cols(c)
    if cols is None:
        return worst_ratio(after, b, e)
    cb, f = _compact(c, after, b, cols)
    return worst_ratio(f, cb, e)


# ---------------------------------------------------------------------------------------------------- the helpers' cases
BITS2_ROWS, BITS2_COLS = (1, 63, 64, 65, 130), (8, 248, 256, 264)
TILE_LIST_M = (1, 63, 64, 65, 4096, 4097, 8200)
TILE_FLAGS = ((64, 193), (128, 385), (256, 700), (300, 1000))
ROWS_MASK_COLS = (8, 2048, 2056)
CONCAT = tuple((r1, r2, rows) for r1, r2 in ((8, 8), (8, 256), (64, 8), (256, 64), (64, 64), (256, 256)) for rows in (1, 4097))


def helper_row_set(M, kind, seed=0):
    g = torch.Generator().manual_seed(M * 13 + seed)
    if kind == "sparse":                                   # a few marked tiles, several in a row, and past the 64th tile when there is one
        m = torch.zeros(M, dtype=U8)
        idx = torch.randint(0, M, (max(1, M // 97),), generator=g)
        m[idx] = 1
        if M > 64 * 70:
            m[64 * 66 + 3] = 1
            m[64 * 64] = 1
        return m
    if kind == "dense":
        return (torch.rand(M, generator=g) < 0.5).to(U8)
    m = torch.zeros(M, dtype=U8)
    if kind == "lasttile":                                 # marks only in the (ragged) last tile
        m[(M - 1) // 64 * 64::2] = 1
        m[M - 1] = 1
    return m
