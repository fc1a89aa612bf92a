"""CPU-only checks of the source-row-map entry points (vlr_rmsnorm_bwd_src, vlr_rmsnorm_bwd_f32_src, vlr_swiglu_bwd_src,
vlr_gemm_swiglu_bwd_src, vlr_decoder_layer_fwd_compact_keep, vlr_decoder_layer_bwd_src): declared, exported and bound with the
arity of the header; null arguments, bad shapes and aliased buffers are refused with a message before anything is launched; the
entry points they sit beside keep their error text.  The kernels themselves: tests/test_hip_src_maps.py."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("vlr_rmsnorm_bwd_src", "vlr_rmsnorm_bwd_f32_src", "vlr_swiglu_bwd_src", "vlr_gemm_swiglu_bwd_src",
       "vlr_decoder_layer_fwd_compact_keep", "vlr_decoder_layer_bwd_src")


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
    # the mapped forms take the unmapped argument list plus the map
    assert len(_hip._SIGS["vlr_rmsnorm_bwd_src"]) == len(_hip._SIGS["vlr_rmsnorm_bwd"]) + 1
    assert len(_hip._SIGS["vlr_rmsnorm_bwd_f32_src"]) == len(_hip._SIGS["vlr_rmsnorm_bwd_f32"]) + 1
    assert _hip.helper("vlr_abi_version") == 9               # additive entry points: no caller breaks


def test_null_arguments_and_shapes_are_refused():
    from vlrlhf import _hip
    l = _hip.lib()
    one = C.c_void_p(4096)
    err = lambda: l.vlr_last_error().decode()      # noqa: E731
    # norm backward: the map is required; everything else answers as the unmapped call does
    for name in ("vlr_rmsnorm_bwd_src", "vlr_rmsnorm_bwd_f32_src"):
        f = getattr(l, name)
        assert f(one, one, one, one, None, one, None, 0, one, None, 8, 256, None) == 1 and f"{name}: null row map" in err()
        assert f(None, one, one, one, None, one, None, 0, one, one, 8, 256, None) == 1 and "vlr_rmsnorm_bwd: null argument" in err()
        assert f(one, one, one, one, None, one, None, 0, one, one, 8, 12, None) == 1 and "vlr_rmsnorm_bwd: bad shape" in err()
        assert f(one, one, one, one, None, one, None, 0, one, one, 8, 8200, None) == 1 and "H<=8192" in err()
        assert f(one, one, one, one, None, one, None, 0, None, one, 8, 256, None) == 1 and "workspace" in err()
    assert l.vlr_rmsnorm_bwd(None, one, one, one, None, one, None, 0, one, 8, 256, None) == 1 and "vlr_rmsnorm_bwd: null argument" in err()
    # the unfused SwiGLU backward through a map
    assert l.vlr_swiglu_bwd_src(one, None, one, one, 8, 64, None) == 1 and "vlr_swiglu_bwd_src: null argument" in err()
    assert l.vlr_swiglu_bwd_src(one, one, one, one, 8, 12, None) == 1 and "vlr_swiglu_bwd_src: bad shape" in err()
    assert l.vlr_swiglu_bwd_src(one, one, one, one, 0, 64, None) == 1 and "vlr_swiglu_bwd_src: bad shape" in err()
    # the fused one: every pointer, the shape, and the alias
    g = l.vlr_gemm_swiglu_bwd_src
    two = C.c_void_p(1 << 30)
    for hole in range(6):
        args = [one, one, one, one, two, one]
        args[hole] = None
        assert g(*args, 8, 64, 256, None) == 1 and "vlr_gemm_swiglu_bwd_src: null operand" in err(), hole
    assert g(one, one, one, one, two, one, 8, 60, 256, None) == 1 and "vlr_gemm_swiglu_bwd_src: bad shape M=8 I=60 H=256" in err()
    assert g(one, one, one, one, two, one, 0, 64, 256, None) == 1 and "vlr_gemm_swiglu_bwd_src: bad shape" in err()
    assert l.vlr_gemm_swiglu_bwd(one, one, None, one, 8, 64, 256, None) == 1 and "vlr_gemm_swiglu_bwd: null operand" in err()


def test_aliased_output_is_refused():
    """dgu_out [M][2I] must not hold gu_src: the same pointer, and a source that starts inside the output (M * 2I * 2 bytes)"""
    from vlrlhf import _hip
    l = _hip.lib()
    err = lambda: l.vlr_last_error().decode()      # noqa: E731
    one = C.c_void_p(4096)
    out = 1 << 30
    M, I = 8, 64
    span = M * 2 * I * 2
    for src in (out, out + 256, out + span - 16):
        assert l.vlr_gemm_swiglu_bwd_src(one, one, C.c_void_p(src), one, C.c_void_p(out), one, M, I, 256, None) == 1
        assert "vlr_gemm_swiglu_bwd_src: dgu_out must not alias gu_src" in err(), src


def test_layer_calls_refuse_null_arguments():
    from vlrlhf import _hip
    l = _hip.lib()
    err = lambda: l.vlr_last_error().decode()      # noqa: E731
    assert l.vlr_decoder_layer_fwd_compact_keep(None, None, None, None, None, None, None, 2, 8, None) == 1
    assert "vlr_decoder_layer_fwd_compact_keep: null argument" in err()
    assert l.vlr_decoder_layer_bwd_src(None, None, None, 0, None, None, None, None, None, None, None, None, None, 2, 8, None) == 1
    assert "vlr_decoder_layer_bwd_src: null argument" in err()
    # a row-map struct with a null map, activation sets with a null tensor, and a scratch set that is the layer's own
    cfg = _hip.LlamaCfg(256, 512, 2, 128, 1e-5, 64, None, None, 2, 1)
    lw = _hip.LayerWeights(*([4096] * 6), None)
    acts = _hip.LayerActs(*([4096] * 11))
    other = _hip.LayerActs(*([8192] * 11))
    holes = _hip.LayerActs(*([4096] * 10 + [None]))
    maps = _hip.RowMaps(4096, 4096, 4096, 4096, 4096, 8, 0)
    nomap = _hip.RowMaps(4096, None, 4096, 4096, 4096, 8, 0)
    x = C.c_void_p(4096)
    f = l.vlr_decoder_layer_fwd_compact_keep
    assert f(C.byref(cfg), C.byref(lw), C.byref(acts), C.byref(other), x, C.byref(nomap), None, 2, 8, None) == 1 and "null row map" in err()
    assert f(C.byref(cfg), C.byref(lw), C.byref(holes), C.byref(other), x, C.byref(maps), None, 2, 8, None) == 1 and "null activation pointer" in err()
    assert f(C.byref(cfg), C.byref(lw), C.byref(acts), C.byref(acts), x, C.byref(maps), None, 2, 8, None) == 1 and "must not alias" in err()
    # vlr_layer_acts_expand, which the new forward replaces on the default route, keeps its own messages
    assert l.vlr_layer_acts_expand(None, None, None, None, 8, 1, None) == 1 and "vlr_layer_acts_expand: null argument" in err()


def test_row_map_forward_entry_points():
    """the scatter norms and the A-row-map launches: declared, bound, null arguments refused before anything is launched"""
    from vlrlhf import _hip
    l = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "vlr.h")).read()
    err = lambda: l.vlr_last_error().decode()      # noqa: E731
    one = C.c_void_p(4096)
    for name in ("vlr_rmsnorm_fwd_scatter", "vlr_rmsnorm_fwd_f32_scatter", "vlr_gemm_qkv_rope_bias_rows", "vlr_gemm_swiglu_rows", "vlr_gemm_res_rows"):
        assert hasattr(l, name) and name in _hip.exported_symbols(), name
        assert len(_hip._SIGS[name]) == _proto_args(hdr, name), name
    for name in ("vlr_rmsnorm_fwd_scatter", "vlr_rmsnorm_fwd_f32_scatter"):
        f = getattr(l, name)
        assert f(one, one, one, one, one, None, 8, 256, 1e-5, None) == 1 and f"{name}: null argument" in err()
        assert f(one, one, one, one, None, one, 8, 256, 1e-5, None) == 1 and f"{name}: null argument" in err()
        assert f(one, one, one, one, one, one, 8, 12, 1e-5, None) == 1 and f"{name}: bad shape" in err()
    assert l.vlr_gemm_qkv_rope_bias_rows(one, None, one, None, one, one, one, one, 8, 768, 512, 256, 256, 128, 64, None) == 1
    assert "vlr_gemm_qkv_rope_bias_rows: null row map" in err()
    assert l.vlr_gemm_swiglu_rows(one, None, one, one, one, 8, 512, 256, 256, 1, None) == 1 and "vlr_gemm_swiglu_rows: null row map" in err()
    assert l.vlr_gemm_res_rows(1, one, None, one, one, one, 8, 1024, 256, 0, 0, None) == 1 and "vlr_gemm_res_rows: null argument" in err()
    assert l.vlr_gemm_res_rows(1, one, one, one, one, one, 8, 1024, 256, 8, 0, None) == 1 and "peeled rows" in err()
    assert l.vlr_gemm_res_rows(1, one, one, one, one, one, 8, 1024, 256, 4, -1, None) == 1 and "peeled rows" in err()
    # the unmapped entry points keep their messages
    assert l.vlr_gemm_swiglu(None, one, one, one, 8, 512, 256, 256, 1, None) == 1 and "vlr_gemm_swiglu: null operand" in err()
