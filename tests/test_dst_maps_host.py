"""CPU-only checks of the output-row-map entry points (vlr_gemm_qkv_rope_bias_dst, vlr_gemm_swiglu_dst,
vlr_decoder_layer_fwd_compact_maps): declared, exported and bound with the arity of the header; null maps, null operands and a
destination that is the source are refused with a message before anything is launched; and the twin map of the reference pass's plan
(prefix_dedup.build_twin) against a construction row by row.  The kernels themselves: tests/test_hip_dst_maps.py."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("vlr_gemm_qkv_rope_bias_dst", "vlr_gemm_swiglu_dst", "vlr_decoder_layer_fwd_compact_maps")


def _proto_args(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} has no prototype in include/vlr.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_declared_exported_and_bound():
    from vlrlhf import _hip
    l = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "vlr.h")).read()
    for name in NEW:
        assert hasattr(l, name) and name in _hip.exported_symbols(), name
        assert len(_hip._SIGS[name]) == _proto_args(hdr, name), name
        assert list(getattr(l, name).argtypes) == _hip._SIGS[name], name
    # the unmapped argument list, the A-side map, two output maps and the three fallback arguments
    assert len(_hip._SIGS["vlr_gemm_qkv_rope_bias_dst"]) == len(_hip._SIGS["vlr_gemm_qkv_rope_bias_rows"]) + 5
    assert len(_hip._SIGS["vlr_gemm_swiglu_dst"]) == len(_hip._SIGS["vlr_gemm_swiglu_rows"]) + 5
    assert _hip.helper("vlr_abi_version") == 9               # additive entry points: no caller breaks


def test_null_and_aliased_arguments_are_refused():
    from vlrlhf import _hip
    l = _hip.lib()
    err = lambda: l.vlr_last_error().decode()      # noqa: E731
    one, two, three = C.c_void_p(4096), C.c_void_p(1 << 30), C.c_void_p(1 << 31)
    q = l.vlr_gemm_qkv_rope_bias_dst
    tail = (one, one, one, 8, 768, 512, 256, 256, 128, 64, None)           # pos, cos, sin, M, N, rope_cols, K, ldx, head_dim, max_pos, stream
    assert q(one, None, one, None, two, None, one, None, None, 0, *tail) == 1 and "vlr_gemm_qkv_rope_bias_dst: null output row map" in err()
    assert q(one, None, one, None, two, one, None, None, None, 0, *tail) == 1 and "vlr_gemm_qkv_rope_bias_dst: null output row map" in err()
    for hole in (0, 2, 4):
        args = [one, None, one, None, two, one, one, None, None, 0]
        args[hole] = None
        assert q(*args, *tail) == 1 and "vlr_gemm_qkv_rope_bias_dst: null operand" in err(), hole
    assert q(one, None, one, None, one, one, one, None, None, 0, *tail) == 1 and "must not be the source" in err()
    assert q(one, None, one, None, two, one, one, two, one, 16, *tail) == 1 and "must not be the source or the fallback rows" in err()
    # a shape the fused kernel refuses (K = 128) without the fallback's buffers, or with an A-side map: an error, nothing is launched
    short = (one, one, one, 8, 768, 512, 128, 128, 128, 64, None)
    assert q(one, None, one, None, two, one, one, None, None, 0, *short) == 1 and "the fallback needs" in err()
    assert q(one, one, one, None, two, one, one, three, one, 16, *short) == 1 and "the fallback needs" in err()
    s = l.vlr_gemm_swiglu_dst
    tail = (8, 512, 256, 256, 1, None)                                      # M, I, K, ldx, store_gu, stream
    assert s(one, one, one, three, two, None, one, None, None, 0, *tail) == 1 and "vlr_gemm_swiglu_dst: null output row map" in err()
    assert s(one, one, one, three, two, one, None, None, None, 0, *tail) == 1 and "vlr_gemm_swiglu_dst: null output row map" in err()
    for hole in (0, 2, 3, 4):
        args = [one, one, one, three, two, one, one, None, None, 0]
        args[hole] = None
        assert s(*args, *tail) == 1 and "vlr_gemm_swiglu_dst: null operand" in err(), hole
    assert s(one, one, one, three, one, one, one, None, None, 0, *tail) == 1 and "must not be the source" in err()
    assert s(one, one, one, three, three, one, one, None, None, 0, *tail) == 1 and "must not be the source, gate | up" in err()
    # no A-side map: the mapped SwiGLU kernel does not exist - the fallback, which needs its buffers
    assert s(one, None, one, three, two, one, one, None, None, 0, *tail) == 1 and "the fallback needs" in err()
    f = l.vlr_decoder_layer_fwd_compact_maps
    assert f(None, None, None, None, None, None, None, None, 2, 8, 0, None) == 1 and "vlr_decoder_layer_fwd_compact_maps: null argument" in err()
    cfg = _hip.LlamaCfg(256, 512, 2, 128, 1e-5, 64, None, None, 2, 1)
    lw = _hip.LayerWeights(*([4096] * 6), None)
    acts = _hip.LayerActs(*([4096] * 11))
    nomap = _hip.RowMaps(4096, None, None, 4096, 4096, 8, 0)
    assert f(C.byref(cfg), C.byref(lw), C.byref(acts), one, C.byref(nomap), two, two, None, 2, 8, 0, None) == 1 and "null row map" in err()
    # the entry points they sit beside keep their messages
    assert l.vlr_gemm_swiglu_rows(one, None, one, one, one, 8, 512, 256, 256, 1, None) == 1 and "vlr_gemm_swiglu_rows: null row map" in err()


def _twin_by_rows(P, S):
    """row by row: kept row j stands at dense row compact_rows[j]; the dropped row (B + i) * S + s, s < P_i, is the twin of the kept
    row that stands at i * S + s"""
    B = len(P)
    kept = [b * S + s for b in range(2 * B) for s in range(S) if b < B or s >= P[b - B]]
    where = {d: j for j, d in enumerate(kept)}
    twin = [-1] * len(kept)
    for i, p in enumerate(P):
        for s in range(p):
            twin[where[i * S + s]] = (B + i) * S + s
    return kept, twin


@pytest.mark.parametrize("P,S", [([1, 90, 43], 90), ([0, 7], 7), ([5], 5), ([0], 3), ([3, 0, 11, 2], 11), ([201, 201], 805)])
def test_reference_plan_twin(P, S):
    from vlrlhf import prefix_dedup as PD
    rows, dsrc = PD.build_row_maps(P, S)
    twin = PD.build_twin(rows, dsrc)
    kept, want = _twin_by_rows(P, S)
    assert rows.tolist() == kept and twin.dtype == torch.int32 and twin.tolist() == want
    # every dense row is written exactly once: by its own kept row or as a twin
    M = 2 * len(P) * S
    written = sorted(kept + [t for t in want if t >= 0])
    assert written == list(range(M))
    # and it is the policy plan's twin where the policy plan trims nothing
    plan = PD.build_policy_plan(P, S)
    if plan["P"] == list(P):
        assert plan["twin"].tolist() == want
