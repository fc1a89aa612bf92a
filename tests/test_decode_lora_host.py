"""CPU-only checks of decoding with live LoRA adapters: the header declares the new entry points and the library exports them (ABI
version unchanged), the ctypes signatures match the prototypes, argument errors are reported without a GPU, the target-block index
rule of the adapter slice matches LoraLayout's fused row order, and generate() routes merged / live / plain as documented."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.golden_util import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vlr_gemv_lora_workspace_bytes", "vlr_gemv_lora_u_bytes", "vlr_gemv_bf16_lora", "vlr_gemv_w4_lora", "vlr_decoder_layer_decode_lora",
       "vlr_decoder_layer_decode_w4_lora"]


def header():
    return open(os.path.join(ROOT, "include", "vlr.h")).read()


def prototype_args(hdr, name):
    """number of parameters of the prototype `name(...)` in include/vlr.h"""
    m = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} has no prototype in include/vlr.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_declares_and_library_exports_the_entry_points():
    from vlrlhf import _hip
    l = _hip.lib()
    hdr = header()
    declared = set(re.findall(r"\b(vlr_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} not declared in include/vlr.h"
        assert hasattr(l, name), f"{name} declared but not exported by libvlr_hip.so"
        assert name in _hip.exported_symbols()
    assert "vlr_decode_lora_ws" in hdr
    assert _hip.helper("vlr_abi_version") == 9               # additive entry points: no caller breaks


def test_ctypes_signatures_match_the_prototypes():
    from vlrlhf import _hip
    l = _hip.lib()
    hdr = header()
    for name in NEW[2:]:
        assert len(_hip._SIGS[name]) == prototype_args(hdr, name), name
        assert list(getattr(l, name).argtypes) == _hip._SIGS[name]
    for name in NEW[:2]:
        fn = getattr(l, name)
        assert fn.restype is _hip.C.c_long and len(fn.argtypes) == prototype_args(hdr, name)
    # the adapter entry points are the adapter-free signatures + (A, B, r, targets, outs, scale, u) in front of the stream
    extra = [_hip.P, _hip.P, _hip.I, _hip.I, _hip.P, _hip.F, _hip.P]
    for base in ("vlr_gemv_bf16", "vlr_gemv_w4"):
        assert _hip._SIGS[base + "_lora"] == _hip._SIGS[base][:-1] + extra + [_hip.P]
    assert [f for f, _ in _hip.DecodeLoraWs._fields_] == ["u", "u_bytes"]
    assert [f for f, _ in _hip.DecodeWs._fields_] == ["xn", "rstd", "qkv", "attn", "act", "gemv_ws", "gemv_ws_bytes", "attn_ws", "attn_ws_bytes"]


def test_argument_errors_and_sizes_without_gpu():
    from vlrlhf import _hip
    l = _hip.lib()
    # one more fp32 slice than the adapter-free workspace of the form that splits K further; the u scratch is a skinny-GEMM workspace
    for M, N, K, rt in ((4, 12288, 4096, 384), (16, 4096, 11008, 128), (1, 64, 128, 8), (4, 200, 136, 16)):
        plain = max(l.vlr_gemv_workspace_bytes(M, N, K), l.vlr_gemv_w4_workspace_bytes(M, N, K))
        assert l.vlr_gemv_lora_workspace_bytes(M, N, K, rt) == plain + M * N * 4
        assert l.vlr_gemv_lora_u_bytes(M, K, rt) == l.vlr_gemv_workspace_bytes(M, rt, K) > 0
    assert l.vlr_gemv_lora_workspace_bytes(4, 64, 128, 12) == 0
    one = 16                                                  # a non-null, 16-byte aligned stand-in pointer: the checks never read it
    args = [0, one, 128, one, one, 64, None, None, 0, None, None, None, 0, 128, 0, 4, 64, 128, one]
    assert l.vlr_gemv_bf16_lora(*args, one, one, 12, 1, None, 1.0, one, None) == 1
    assert b"vlr_gemv_bf16_lora" in l.vlr_last_error() and b"multiple of 8" in l.vlr_last_error()
    args[15] = 17
    assert l.vlr_gemv_bf16_lora(*args, one, one, 8, 1, None, 1.0, one, None) == 1
    assert b"1 <= M <= 16" in l.vlr_last_error()
    args[15] = 4
    assert l.vlr_gemv_bf16_lora(*args, one, one, 8, 1, None, 1.0, None, None) == 1
    assert b"null adapter" in l.vlr_last_error()
    assert l.vlr_gemv_bf16_lora(*args, one, one, 8, 3, None, 1.0, one, None) == 1
    assert b"not a multiple of targets" in l.vlr_last_error()
    w4 = [0, one, 128, one, one, one, 32, one, 64, None, None, 0, None, None, None, 0, 128, 0, 4, 64, 128, one]
    assert l.vlr_gemv_w4_lora(*w4, one, one, 20, 1, None, 1.0, one, None) == 1
    assert b"vlr_gemv_w4_lora" in l.vlr_last_error() and b"multiple of 8" in l.vlr_last_error()
    assert l.vlr_gemv_w4_lora(*w4, one, one, 8, 5, None, 1.0, one, None) == 1
    assert b"targets" in l.vlr_last_error()
    assert l.vlr_decoder_layer_decode_lora(None, None, None, None, None, None, None, None, None, None, 1, 8, 0, None) == 1
    assert b"vlr_decoder_layer_decode_lora" in l.vlr_last_error()
    assert l.vlr_decoder_layer_decode_w4_lora(None, None, None, None, None, None, None, None, None, None, None, 1, 8, 0, None) == 1
    assert b"vlr_decoder_layer_decode_w4_lora" in l.vlr_last_error()


def target_of_row(n, edges):
    """the device rule (csrc/decode.hip lora_target): t(n) = (n >= n1) + (n >= n2) + (n >= n3), edges beyond the last target = N.
    A re-statement in numpy, not bound to the device code: the test below pins the LAYOUT side (which rows and which A block a
    sub-target owns); the device rule itself is pinned on the GPU (tests/test_hip_decode_lora_kernels.py, the wrong-block test)."""
    e = list(edges[1:]) + [edges[-1]] * (4 - len(edges))
    return (n >= e[0]).astype(int) + (n >= e[1]).astype(int) + (n >= e[2]).astype(int)


@pytest.mark.parametrize("name", ["llava_hipsmall", "llavanext_small"])
def test_target_block_rule_matches_lora_layout(name):
    """row n of a fused lora_B belongs to the sub-target whose lora_A block sits at rows t r .. t r + r - 1 of the fused A: the split the
    layer driver passes (q | k | v = Nq | Nkv | Nkv, gate | up halves, one block for o and down) replayed against LoraLayout.hf_names()"""
    from vlrlhf.engine import LoraLayout
    cfg = load_case(name)[1]
    r = 8
    lay = LoraLayout(cfg, r)
    nh = cfg["heads"]
    nkv = cfg.get("kv_heads") or nh
    hd = cfg.get("head_dim") or cfg["hidden"] // nh
    Nq, Nkv, I, H = nh * hd, nkv * hd, cfg["inter"], cfg["hidden"]
    if name == "llavanext_small":
        assert Nkv < Nq, "the grouped-query case"
    splits = dict(qkv=(Nq, Nkv, Nkv), o=(H,), gu=(I, I), down=(H,))
    names = lay.hf_names()
    seen = 0
    for g, _, targets in lay.groups:
        edges = np.cumsum((0,) + splits[g])
        assert lay.shape[f"l0.b_{g}"] == (edges[-1], r) and lay.shape[f"l0.a_{g}"][0] == len(targets) * r
        for i, t in enumerate(targets):
            mod = "self_attn" if g in ("qkv", "o") else "mlp"
            ka, alo, ahi = names[f"{lay.prefix}0.{mod}.{t}.lora_A.weight"]
            kb, blo, bhi = names[f"{lay.prefix}0.{mod}.{t}.lora_B.weight"]
            assert (ka, kb) == (f"l0.a_{g}", f"l0.b_{g}") and (alo, ahi) == (i * r, (i + 1) * r)
            rows = np.arange(blo, bhi)
            assert (target_of_row(rows, edges) == i).all(), (g, t)
            assert (target_of_row(rows, edges) * r == alo).all()
            seen += 1
    assert seen == 7


class StubModel:
    """what LlavaForRL.generate touches before it picks a path"""

    def __init__(self, packed, lora, active, own_weights=True):
        pol = SimpleNamespace(v={"lm_head": None})
        self.engine = SimpleNamespace(dev=torch.device("cpu"), supports_kv_cache=True, hd=128, policy=pol, lora=lora, lora_active=active,
                                      packed={} if packed else None)
        self.weights = pol if own_weights else SimpleNamespace(v={"lm_head": None})
        self.config, self.training, self.routes = {}, False, []

    is_packed = property(lambda self: self.engine.packed is not None)

    def eval(self):
        pass

    def train(self, mode=True):
        pass

    def cached_lora_route(self, merge_lora=True):
        from vlrlhf.models.Llava import LlavaForRL
        return LlavaForRL.cached_lora_route(self, merge_lora)

    def _generate_cached(self, ids, *a):
        self.routes.append(a[-1])
        return ids


@pytest.mark.parametrize("packed,lora,active,own,kw,route", [
    (False, {"r": 8}, True, True, {}, "merged"),                          # bf16 base, default merge_lora
    (False, {"r": 8}, True, True, {"merge_lora": True}, "merged"),
    (False, {"r": 8}, True, True, {"merge_lora": False}, "live"),
    (False, {"r": 256}, True, True, {"merge_lora": False}, "live"),      # no rank limit on the live path: q|k|v at r = 256 too
    (True, {"r": 256}, True, True, {}, "live"),
    (True, {"r": 8}, True, True, {}, "live"),                             # packed base: nothing to merge, whatever merge_lora says
    (True, {"r": 8}, True, True, {"merge_lora": True}, "live"),
    (True, {"r": 8}, True, True, {"merge_lora": False}, "live"),
    (False, {"r": 8}, False, True, {"merge_lora": False}, "plain"),       # disable_adapter()
    (True, {"r": 8}, False, True, {}, "plain"),
    (False, None, True, True, {"merge_lora": False}, "plain"),            # no adapters at all
    (False, {"r": 8}, True, False, {}, "plain"),                          # a reference model's own weight set
])
def test_generate_routing_table(packed, lora, active, own, kw, route):
    from vlrlhf.models.Llava import LlavaForRL
    m = StubModel(packed, lora, active, own)
    ids = torch.zeros(2, 4, dtype=torch.long)
    out = LlavaForRL.generate(m, input_ids=ids, max_new_tokens=2, **kw)
    assert m.routes == [route] and out.shape == ids.shape
    m.routes.clear()
    LlavaForRL.generate(m, input_ids=ids, max_new_tokens=0, use_cache=False, **kw)       # the re-forward loop never asks
    assert m.routes == []


def test_get_batch_samples_samples_the_policy_unmerged():
    """sampling inside training must not clone the policy: the policy call carries merge_lora=False"""
    from vlrlhf.base.trainer import VLDPOTrainer
    calls = []

    class M:
        def generate(self, **kw):
            calls.append(kw)
            return kw["input_ids"]

    tok = SimpleNamespace(pad_token_id=0, eos_token_id=2, batch_decode=lambda ids, skip_special_tokens=True: ["x"] * ids.shape[0])
    tr = SimpleNamespace(max_length=6, tokenizer=tok, ref_model=M())
    batch = dict(prompt_input_ids=torch.ones(2, 4, dtype=torch.long), prompt_attention_mask=torch.ones(2, 4, dtype=torch.long))
    VLDPOTrainer.get_batch_samples(tr, M(), batch)
    assert calls[0].get("merge_lora") is False and "merge_lora" not in calls[1]


def _kernel_cases():
    import itertools
    from tests import test_hip_decode_lora_kernels as T
    for mode in (T.BF16, T.F32RES, T.SWIGLU):
        for M, (K, N), r in itertools.product((1, 4, 16), T.SHAPES, (8, 16, 64)):
            yield mode, M, K, N, r, None
    for M, K, r in itertools.product((1, 4, 16), (128, 136, 512), (8, 16, 64)):
        yield T.ROPE, M, K, sum(T.QKV), r, None
    for mode in (T.BF16, T.F32RES, T.ROPE, T.SWIGLU):
        for g in (32, -1):
            yield mode, 4, 512, 384, 16, g
    for c in T.BIG_RANK:
        yield c


def test_kernel_test_inputs_separate_a_missing_term_from_rounding():
    """every case of tests/test_hip_decode_lora_kernels.py, on the host: the adapter term of the fp64 reference is at least 10 x the
    mode's tolerance, and the reference recomputed with u left unrounded stays inside half that tolerance of the rounded one"""
    from tests import test_hip_decode_lora_kernels as T
    n = 0
    for mode, M, K, N, r, g in _kernel_cases():
        T.check_inputs(mode, T.case(mode, M, K, N, r, g))
        n += 1
    assert n == 3 * 27 + 27 + 8 + len(T.BIG_RANK)
