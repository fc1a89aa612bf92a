"""CPU-only checks of the row-compact POLICY pass's row maps (vlrlhf/prefix_dedup.py build_policy_plan) on hand-made prefix lists, the
exports of its entry points, and the torch restatement of the two row copies that tests/test_hip_prefix_dedup_policy.py compares the
kernels with."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def expand_rows_zero_ref(src, dense_own):
    """vlr_expand_rows_zero: dense row m = src row dense_own[m], zeros where dense_own[m] < 0"""
    own = dense_own.long()
    out = src[own.clamp(min=0)].clone()
    out[own < 0] = 0
    return out


def fold_rows_ref(src, compact_rows, twin):
    """vlr_fold_rows: row j = src row compact_rows[j] (+ src row twin[j] where twin[j] >= 0: fp32 add, one rounding to nearest even)"""
    tw = twin.long()
    out = src[compact_rows.long()].clone()
    has = tw >= 0
    out[has] = (out[has].float() + src[tw[has]].float()).to(src.dtype)
    return out


CASES = {                    # name -> (P, S)
    "no_prefix": ([0, 0], 10),
    "whole_sequence": ([9, 9], 9),
    "off_the_8_row_boundary": ([5, 3, 7], 11),
    "last_pair_below_the_trim": ([6, 2], 7),       # M - sum P = 20: four rows to keep again, the last pair has two
    "single_pair": ([13], 24),
    "mixed": ([1, 40, 19], 40),
}


@pytest.mark.parametrize("name", list(CASES))
def test_policy_plan_invariants(name):
    from vlrlhf import prefix_dedup as PD
    P, S = CASES[name]
    B, M = len(P), 2 * len(P) * S
    ref_rows, ref_src = PD.build_row_maps(P, S)
    plan = PD.build_policy_plan(P, S)
    # the reference plan of the same prefixes is what it was (and is not touched by the call)
    again_rows, again_src = PD.build_row_maps(P, S)
    assert torch.equal(ref_rows, again_rows) and torch.equal(ref_src, again_src)
    assert ref_rows.numel() == M - sum(P)
    # the trim: at most 7 rows in all, the last pair's first (what it lacks comes from the pair before it), never below 0
    Pt = plan["P"]
    trim_wanted = (-(M - sum(P))) % 8
    assert all(0 <= b <= a for a, b in zip(P, Pt)) and sum(P) - sum(Pt) == trim_wanted <= 7
    assert P[-1] - Pt[-1] == min(trim_wanted, P[-1])
    if name == "last_pair_below_the_trim":
        assert Pt == [4, 0]
    else:
        assert Pt[:-1] == list(P[:-1])
    rows, dsrc, own, twin = plan["compact_rows"], plan["dense_src"], plan["dense_own"], plan["twin"]
    Mc = plan["Mc"]
    assert plan["M"] == M and Mc == M - sum(Pt) == rows.numel() and plan["shared"] == sum(Pt) and plan["tail"] == S - Pt[-1]
    assert Mc % 8 == 0
    assert all(x.dtype == torch.int32 for x in (rows, dsrc, own, twin))
    assert tuple(dsrc.shape) == (M,) and tuple(own.shape) == (M,) and tuple(twin.shape) == (Mc,)
    # the maps agree with the reference builder on the trimmed prefixes
    r2, s2 = PD.build_row_maps(Pt, S)
    assert torch.equal(rows, r2) and torch.equal(dsrc, s2)
    # dense_own[compact_rows[j]] == j; dropped rows are exactly the -1 entries; kept + dropped partition the M rows
    assert torch.equal(own[rows.long()].long(), torch.arange(Mc))
    dropped = sorted((B + i) * S + s for i in range(B) for s in range(Pt[i]))
    assert torch.nonzero(own < 0).reshape(-1).tolist() == dropped
    assert sorted(rows.tolist() + dropped) == list(range(M)) and len(set(rows.tolist())) == Mc
    # twin names exactly the dropped rows, each once, at the compact row of its chosen copy
    named = twin[twin >= 0].tolist()
    assert sorted(named) == dropped
    for j in torch.nonzero(twin >= 0).reshape(-1).tolist():
        d = int(twin[j])
        assert int(rows[j]) == d - B * S and int(dsrc[d]) == j
    # the tail: the last dense rows are kept, and stand last in the compact order
    tail = plan["tail"]
    assert rows[Mc - tail:].tolist() == list(range(M - tail, M))


def test_policy_plan_refuses_bad_prefixes():
    from vlrlhf import prefix_dedup as PD
    for P, S in (([], 4), ([5], 4), ([-1, 2], 4), ([1], 0)):
        with pytest.raises(ValueError, match="build_policy_plan"):
            PD.build_policy_plan(P, S)


def test_restatement_of_expand_and_fold():
    """expand is the adjoint of the dense_src gather on the kept rows; fold(expand(x)) == x; fold sums a pair in fp32 and rounds once"""
    from vlrlhf import prefix_dedup as PD
    plan = PD.build_policy_plan([5, 3, 7], 11)
    Mc, M = plan["Mc"], plan["M"]
    x = torch.randn(Mc, 16).bfloat16()
    d = expand_rows_zero_ref(x, plan["dense_own"])
    assert tuple(d.shape) == (M, 16) and bool((d[plan["dense_own"] < 0] == 0).all())
    assert torch.equal(fold_rows_ref(d, plan["compact_rows"], plan["twin"]), x)
    y = torch.randn(M, 16).bfloat16()
    f = fold_rows_ref(y, plan["compact_rows"], plan["twin"])
    j = int(torch.nonzero(plan["twin"] >= 0)[0])
    a, b = y[int(plan["compact_rows"][j])].double(), y[int(plan["twin"][j])].double()
    assert torch.equal(f[j], (a + b).float().bfloat16())               # two bf16 addends: their fp32 sum is exact before the rounding
    k = int(torch.nonzero(plan["twin"] < 0)[0])
    assert torch.equal(f[k], y[int(plan["compact_rows"][k])])
    # <d y, expand(x)> == <fold(d y), x>: fold is the transpose of the gather the forward applies (up to its one rounding)
    lhs = float((y.double() * x[plan["dense_src"].long()].double()).sum())
    g = torch.zeros(Mc, 16, dtype=torch.float64).index_add_(0, plan["dense_src"].long(), y.double())
    assert abs(lhs - float((g * x.double()).sum())) < 1e-9 * max(1.0, abs(lhs))
    assert float((g - f.double()).abs().max()) <= 2.0 ** -8 * float(g.abs().max())


def test_entry_points_are_declared_exported_and_bound():
    import ctypes as C
    from vlrlhf import _hip
    l = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "vlr.h")).read()
    for name in ("vlr_expand_rows_zero", "vlr_fold_rows", "vlr_decoder_layer_fwd_compact_ex", "vlr_decoder_layer_bwd_compact",
                 "vlr_decoder_layer_compact_exact", "vlr_layer_acts_expand", "vlr_gather_f32"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert hasattr(l, name) and name in _hip.exported_symbols(), name
    assert _hip.helper("vlr_abi_version") == 9               # additive entry points: no caller breaks
    # argument errors come back as VLR_ERR_ARG with a message, before anything is launched
    assert l.vlr_expand_rows_zero(None, None, None, 4, 8, None) == 1 and b"vlr_expand_rows_zero: null argument" in l.vlr_last_error()
    assert l.vlr_fold_rows(None, None, None, None, 4, 8, None) == 1 and b"vlr_fold_rows: null argument" in l.vlr_last_error()
    one = C.c_void_p(16)
    assert l.vlr_expand_rows_zero(one, one, one, 4, 12, None) == 1 and b"multiple of 8" in l.vlr_last_error()
    assert l.vlr_fold_rows(one, one, one, one, 0, 8, None) == 1 and b"vlr_fold_rows: bad shape" in l.vlr_last_error()
    assert l.vlr_decoder_layer_bwd_compact(None, None, None, 0, None, None, None, None, None, None, None, None, 2, 8, None) == 1
    assert b"vlr_decoder_layer_bwd_compact: null argument" in l.vlr_last_error()
    assert l.vlr_layer_acts_expand(None, None, None, None, 8, 1, None) == 1 and b"vlr_layer_acts_expand: null argument" in l.vlr_last_error()
    assert l.vlr_gather_f32(None, None, None, 0, None) == 1 and b"vlr_gather_f32" in l.vlr_last_error()
    # the exactness helper is host arithmetic: out-of-range arguments and the toy widths say 0
    cfg = _hip.LlamaCfg(256, 512, 2, 128, 1e-5, 64, None, None, 2, 1)
    h = lambda *a: _hip.helper("vlr_decoder_layer_compact_exact", *a)      # noqa: E731
    assert h(None, 4, 64, 128, 8) == 0
    assert h(C.byref(cfg), 4, 64, 0, 0) == 0 and h(C.byref(cfg), 4, 64, 257, 0) == 0 and h(C.byref(cfg), 4, 64, 128, 129) == 0
    assert h(C.byref(cfg), 4, 64, 128, 8) == 0               # hidden 256: the residual projections never reach the persistent kernel
