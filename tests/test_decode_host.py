"""CPU-only checks of the KV-cache decoding surface: every new entry point is exported, declared and bound, argument errors come back as
VLR_ERR_ARG with a message before anything launches, and the KVCache position / capacity rule holds on hand-made left-padded masks."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vlr_gemv_bf16", "vlr_gemv_workspace_bytes", "vlr_kv_cache_write", "vlr_attn_decode_gqa", "vlr_attn_decode_workspace_bytes",
       "vlr_decoder_layer_decode"]
FAKE = C.c_void_p(1 << 20)      # never dereferenced: every call below fails validation first


def test_decode_entries_exported_declared_and_bound():
    from vlrlhf import _hip
    l = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "vlr.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} not declared in include/vlr.h"
        assert hasattr(l, name), f"{name} not exported by libvlr_hip.so"
        assert name in _hip.exported_symbols()
    assert "vlr_decode_ws" in hdr and [f for f, _ in _hip.DecodeWs._fields_][:5] == ["xn", "rstd", "qkv", "attn", "act"]
    assert _hip.helper("vlr_abi_version") == 9
    assert l.vlr_gemv_workspace_bytes(4, 4096, 4096) > 0 and l.vlr_gemv_workspace_bytes(17, 4096, 4096) > 0
    assert l.vlr_attn_decode_workspace_bytes(4, 32, 1727) >= 4 * 32 * ((1727 + 63) // 64) * 128 * 4


def _err(rc, l, *words):
    assert rc == 1, rc
    msg = l.vlr_last_error().decode()
    for w in words:
        assert w in msg, msg


def test_decode_argument_errors_without_gpu():
    from vlrlhf import _hip
    l = _hip.lib()
    g = lambda mode, M, N, K, ldx=None: l.vlr_gemv_bf16(mode, FAKE, ldx or K, FAKE, FAKE, N, None, None, 0, None, None, None, 0, 128,  # noqa: E731
                                                       0, M, N, K, FAKE, None)
    _err(g(0, 17, 64, 64), l, "M = 17")
    _err(g(0, 0, 64, 64), l, "M = 0")
    _err(g(0, 4, 64, 60), l, "K = 60", "multiple of 8")
    _err(g(7, 4, 64, 64), l, "mode")
    _err(g(3, 4, 384, 128), l, "RoPE")                           # no tables
    _err(l.vlr_gemv_bf16(0, None, 64, FAKE, FAKE, 64, None, None, 0, None, None, None, 0, 128, 0, 4, 64, 64, FAKE, None), l, "null")
    # decode attention: head_dim 128 only, 1 <= len <= cap
    a = lambda hd, cap, ln, nh=4, nkv=2: l.vlr_attn_decode_gqa(FAKE, 1024, FAKE, FAKE, FAKE, FAKE, 512, FAKE, 2, nh, nkv, hd,  # noqa: E731
                                                              cap, ln, C.c_float(0.1), None)
    _err(a(64, 100, 10), l, "head_dim")
    _err(a(128, 100, 101), l, "len 101")
    _err(a(128, 100, 0), l, "len 0")
    _err(a(128, 100, 10, nh=4, nkv=3), l, "kv_heads")
    # cache write: columns inside the capacity
    _err(l.vlr_kv_cache_write(FAKE, FAKE, 768, FAKE, FAKE, 2, 5, 2, 128, 64, 60, None), l, "capacity")
    # the composed layer: head_dim, len < cap, null arguments
    cfg = _hip.LlamaCfg(4096, 11008, 32, 128, 1e-5, 4096, None, None, 32, 1)
    w = _hip.LayerWeights(*([1 << 20] * 6), None)
    ws = _hip.DecodeWs(*([1 << 20] * 5), 1 << 20, 1 << 30, 1 << 20, 1 << 30)
    lay = lambda c, ln, cap: l.vlr_decoder_layer_decode(C.byref(c), C.byref(w), C.byref(ws), FAKE, FAKE, FAKE, FAKE, FAKE, 4, cap, ln, None)  # noqa: E731
    _err(lay(cfg, 64, 64), l, "len 64", "cap 64")
    _err(lay(cfg, 70, 64), l, "cap")
    cfg96 = _hip.LlamaCfg(3072, 8192, 32, 96, 1e-5, 4096, None, None, 32, 1)
    _err(lay(cfg96, 10, 64), l, "head_dim 96")
    small = _hip.DecodeWs(*([1 << 20] * 5), 1 << 20, 16, 1 << 20, 1 << 30)
    _err(l.vlr_decoder_layer_decode(C.byref(cfg), C.byref(w), C.byref(small), FAKE, FAKE, FAKE, FAKE, FAKE, 4, 64, 10, None), l, "gemv_ws")
    _err(l.vlr_decoder_layer_decode(C.byref(cfg), C.byref(w), C.byref(ws), None, FAKE, FAKE, FAKE, FAKE, 4, 64, 10, None), l, "null")


def test_kv_cache_position_and_capacity_rule():
    """the merge's positions are cumsum(mask) - 1 on the attended rows, so the token appended next takes the number of attended
    columns of its row; every decode step adds one attended column to every row (finished rows included, as the re-forward loop
    does), and the capacity is the merged prompt plus the new-token budget"""
    from vlrlhf.engine import KVCache
    mask = torch.tensor([[1, 1, 1, 1, 1, 1],
                         [0, 0, 1, 1, 1, 1],
                         [0, 0, 0, 0, 0, 1]], dtype=torch.int32)
    merged_pos = (mask.cumsum(1) - 1) * mask + (1 - mask)          # the merge's rule (padded rows hold 1)
    c = KVCache(layers=2, batch=3, kv_heads=1, head_dim=128, new_tokens=4, device="cpu")
    assert c.reserve(6, alloc=False) == KVCache.capacity(6, 4) == 10
    c.start(mask)
    assert c.len == 6
    assert c.pos.tolist() == [6, 4, 1]
    assert c.pos.tolist() == [int(merged_pos[b][mask[b] != 0].max()) + 1 for b in range(3)]
    assert KVCache.next_positions(c.key_mask, c.len).tolist() == [6, 4, 1]
    for step in range(4):
        col = c.open_column()
        assert col == 6 + step and c.key_mask[:, col].tolist() == [1, 1, 1]
        c.advance()
        assert c.pos.tolist() == [7 + step, 5 + step, 2 + step]
        assert KVCache.next_positions(c.key_mask, c.len).tolist() == c.pos.tolist()
    assert c.key_mask[1].tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 1, 1]
    with pytest.raises(ValueError, match="full"):
        c.open_column()
    c2 = KVCache(layers=1, batch=1, kv_heads=1, head_dim=128, new_tokens=0, device="cpu")
    c2.reserve(4, alloc=False)
    with pytest.raises(ValueError, match="capacity"):
        c2.start(torch.ones(1, 5, dtype=torch.int32))


def test_engine_flags_select_the_cached_path():
    from vlrlhf.engine import LlavaHipEngine
    from vlrlhf.engine_internlm import InternLMHipEngine
    from vlrlhf.engine_qwen import QwenVLHipEngine
    assert LlavaHipEngine.supports_kv_cache is True
    assert QwenVLHipEngine.supports_kv_cache is False and InternLMHipEngine.supports_kv_cache is False
    import inspect
    from vlrlhf.models.Llava import LlavaForRL
    assert inspect.signature(LlavaForRL.generate).parameters["use_cache"].default is True
    assert "kv_cache" in inspect.signature(LlavaHipEngine.forward_hidden).parameters
