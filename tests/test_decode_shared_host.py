"""CPU-only checks of num_return_sequences over a shared prompt cache: SharedPromptKVCache bookkeeping, generate()'s pickup of
generation_config.num_return_sequences and its refusal of greedy search with several sequences (on a stub engine), the new entry points'
argument errors without a GPU, and the unchanged ABI version."""
import re
import os
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vlr_attn_decode_shared_workspace_bytes", "vlr_attn_decode_shared", "vlr_decoder_layer_decode_shared"]


def test_header_declares_and_library_exports_the_entry_points():
    from vlrlhf import _hip
    l = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "vlr.h")).read()
    declared = set(re.findall(r"\b(vlr_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and hasattr(l, name) and name in _hip.exported_symbols(), name
    assert _hip.helper("vlr_abi_version") == 9               # additive entry points: no caller breaks
    m = re.search(r"typedef struct \{([^}]*)\} vlr_kv_shared;", hdr, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [f.strip().lstrip("*") for decl in body.split(";") for f in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", decl).split(",") if f.strip()]
    assert fields == [f for f, _ in _hip.KvShared._fields_]
    for name in NEW[1:]:
        proto = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", hdr, re.S).group(1)
        assert len(_hip._SIGS[name]) == len([a for a in proto.split(",") if a.strip()]), name


def test_shared_cache_bookkeeping():
    from vlrlhf.engine import KVCache, SharedPromptKVCache
    c = SharedPromptKVCache(layers=2, prompts=2, fanout=3, kv_heads=1, head_dim=128, new_tokens=2, device="cpu")
    assert isinstance(c.prompt, KVCache) and c.prompt.new_tokens == 0 and c.B == 6
    with pytest.raises(ValueError, match="begin"):
        c.open_column()
    c.prompt.reserve(5, alloc=False)                          # the prefill: 5 merged rows, the second prompt left-padded by 2
    assert c.prompt.cap == 5 and c.cap == 7
    with pytest.raises(ValueError, match="empty"):
        c.begin(alloc=False)
    c.prompt.start(torch.tensor([[1, 1, 1, 1, 1], [0, 0, 1, 1, 1]]))
    c.begin()
    assert c.pos.tolist() == [5, 5, 5, 3, 3, 3] and c.pos.dtype == torch.int32
    assert c.k_tail.shape == c.v_tail.shape == (2, 6, 1, 2, 128) and c.k_tail.dtype == torch.bfloat16
    assert (c.tail_cap, c.tail_len, c.len) == (2, 0, 5)
    assert c.nbytes() == 2 * 2 * 2 * 128 * (2 * 5 + 6 * 2)
    assert c.open_column() == 0
    c.advance()
    assert c.open_column() == 1 and c.pos.tolist() == [6, 6, 6, 4, 4, 4]
    c.advance()
    assert (c.tail_len, c.len) == (2, 7) and c.prompt.len == 5 and c.prompt.pos.tolist() == [5, 3]
    with pytest.raises(ValueError, match="full"):
        c.open_column()
    with pytest.raises(ValueError, match="fanout"):
        SharedPromptKVCache(2, 2, 0, 1, 128, 2, device="cpu")


class StubModel:
    """what LlavaForRL.generate touches before it picks a path (tests/test_decode_lora_host.py's stub, recording the fan-out)"""

    def __init__(self, supports=True):
        pol = SimpleNamespace(v={"lm_head": None})
        self.engine = SimpleNamespace(dev=torch.device("cpu"), supports_kv_cache=supports, hd=128, policy=pol, lora=None, lora_active=False,
                                      packed=None)
        self.weights = pol
        self.config, self.training, self.seen = {}, False, []

    is_packed = False

    def eval(self):
        pass

    def train(self, mode=True):
        pass

    def cached_lora_route(self, merge_lora=True):
        return "plain"

    def _generate_cached(self, ids, *a, **k):
        self.seen.append(k)
        return ids.repeat_interleave(k.get("fanout", 1), 0)

    @staticmethod
    def _expand_rows(v, B, n):
        from vlrlhf.models.Llava import LlavaForRL
        return LlavaForRL._expand_rows(v, B, n)


def test_num_return_sequences_pickup_and_refusal():
    from vlrlhf.models.Llava import LlavaForRL
    ids = torch.zeros(2, 4, dtype=torch.long)
    m = StubModel()
    out = LlavaForRL.generate(m, input_ids=ids, max_new_tokens=2, do_sample=True, num_return_sequences=3)
    assert m.seen == [{"fanout": 3}] and out.shape == (6, 4)
    m.seen.clear()
    LlavaForRL.generate(m, input_ids=ids, max_new_tokens=2, do_sample=True)
    LlavaForRL.generate(m, input_ids=ids, max_new_tokens=2, do_sample=True, num_return_sequences=1)
    assert m.seen == [{}, {}], "n == 1 is today's call"
    m.seen.clear()
    gc = SimpleNamespace(do_sample=True, num_return_sequences=4, max_new_tokens=2, use_cache=True)
    LlavaForRL.generate(m, input_ids=ids, generation_config=gc)
    assert m.seen == [{"fanout": 4}]
    for kw in (dict(num_return_sequences=2), dict(num_return_sequences=2, do_sample=False),
               dict(generation_config=SimpleNamespace(do_sample=False, num_return_sequences=2, max_new_tokens=2, use_cache=True))):
        with pytest.raises(ValueError, match="num_return_sequences"):
            LlavaForRL.generate(m, input_ids=ids, max_new_tokens=2, **kw)
    with pytest.raises(ValueError, match="positive"):
        LlavaForRL.generate(m, input_ids=ids, max_new_tokens=2, do_sample=True, num_return_sequences=0)
    # the expansion of the routes without a shared cache: rows in repeat_interleave order, per-prompt lists too
    e = LlavaForRL._expand_rows
    assert e(torch.tensor([[1], [2]]), 2, 3).flatten().tolist() == [1, 1, 1, 2, 2, 2]
    assert e(["a", "b"], 2, 2) == ["a", "a", "b", "b"] and e(7, 2, 2) == 7 and e(torch.zeros(3, 1), 2, 2).shape == (3, 1)


def test_argument_errors_without_gpu():
    from vlrlhf import _hip
    l = _hip.lib()
    assert l.vlr_attn_decode_shared_workspace_bytes(4, 8, 32, 1599, 128) == \
        4 * 8 * 32 * 25 * 132 * 4 + l.vlr_attn_decode_workspace_bytes(32, 32, 128)
    assert l.vlr_attn_decode_shared_workspace_bytes(4, 0, 32, 1599, 128) == 0
    one = 16                                                  # a non-null, 16-byte aligned stand-in pointer: the checks never read it

    def kv(**over):
        f = dict(k_prompt=one, v_prompt=one, prompt_mask=one, prompts=2, prompt_cap=8, prompt_len=8, k_tail=one, v_tail=one, fanout=3,
                 tail_cap=4, tail_len=1)
        f.update(over)
        return _hip.C.byref(_hip.KvShared(**f))

    def attn(kvp, heads=32, kvh=8, hd=128, q=one):
        return l.vlr_attn_decode_shared(q, 4096, kvp, one, 4096, one, heads, kvh, hd, 0.1, None)

    for args, msg in (((None,), b"null argument"), ((kv(), 32, 8, 128, None), b"null argument"), ((kv(k_tail=None),), b"null cache pointer"),
                      ((kv(), 32, 8, 64), b"head_dim 64"), ((kv(), 32, 5), b"not a multiple of kv_heads"),
                      ((kv(prompt_len=0),), b"prompt_len 0"), ((kv(prompt_len=9),), b"prompt_len 9"), ((kv(tail_len=0),), b"tail_len 0"),
                      ((kv(tail_len=5),), b"tail_len 5"), ((kv(fanout=0),), b"fanout 0")):
        assert attn(*args) == 1, msg
        assert b"vlr_attn_decode_shared" in l.vlr_last_error() and msg in l.vlr_last_error(), l.vlr_last_error()
    assert l.vlr_decoder_layer_decode_shared(None, None, None, None, None, None, None, None, None, None) == 1
    assert b"vlr_decoder_layer_decode_shared" in l.vlr_last_error()
    cfg = _hip.LlamaCfg(256, 256, 2, 128, 1e-5, 64, one, one, 1, 0)
    lw = _hip.LayerWeights(one, one, one, one, one, one, None)
    ws = _hip.DecodeWs(one, one, one, one, one, one, 1 << 30, one, 1 << 30)
    layer = lambda kvp, c=cfg: l.vlr_decoder_layer_decode_shared(_hip.C.byref(c), _hip.C.byref(lw), None, None, _hip.C.byref(ws), None, one,  # noqa: E731
                                                                 one, kvp, None)
    for kvp, msg in ((kv(tail_len=5), b"tail_len 5"), (kv(prompt_len=0), b"prompt_len 0"), (kv(fanout=0), b"fanout 0"),
                     (kv(v_prompt=None), b"null cache pointer")):
        assert layer(kvp) == 1
        assert b"vlr_decoder_layer_decode_shared" in l.vlr_last_error() and msg in l.vlr_last_error(), l.vlr_last_error()
    assert layer(kv(), _hip.LlamaCfg(256, 256, 2, 64, 1e-5, 64, one, one, 1, 0)) == 1 and b"head_dim 64" in l.vlr_last_error()
    small = _hip.DecodeWs(one, one, one, one, one, one, 1 << 30, one, 64)
    assert l.vlr_decoder_layer_decode_shared(_hip.C.byref(cfg), _hip.C.byref(lw), None, None, _hip.C.byref(small), None, one, one, kv(), None) == 1
    assert b"attn_ws" in l.vlr_last_error()
