"""CPU-only checks of Qwen-VL's opt-in KV cache: the rotary position of the first decoded token is the engine's rule (the column index
on Qwen-VL, the attended count elsewhere) and reaches KVCache.start and SharedPromptKVCache.begin through the caches the engine makes;
the class default stays on the re-forward loop and enable_kv_cache() touches one engine instance."""
from types import SimpleNamespace

import torch

MASK = torch.tensor([[0, 0, 0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 1, 1], [0, 1, 1, 1, 1, 1, 1, 1]], dtype=torch.int32)      # left-padded


def test_position_hook_column_index_on_qwen_attended_count_elsewhere():
    from vlrlhf.engine import KVCache, LlavaHipEngine
    from vlrlhf.engine_qwen import QwenVLHipEngine
    S = MASK.shape[1]
    q = QwenVLHipEngine.kv_next_positions(MASK, S)
    assert q.dtype == torch.int32 and q.tolist() == [8, 8, 8], "pos = arange(S) in every row: the next token sits at column S"
    assert QwenVLHipEngine.kv_next_positions(MASK, 6).tolist() == [6, 6, 6] and QwenVLHipEngine.kv_next_positions(MASK).tolist() == [8, 8, 8]
    l = LlavaHipEngine.kv_next_positions(MASK, S)
    assert l.dtype == torch.int32 and l.tolist() == [5, 8, 7] == KVCache.next_positions(MASK, S).tolist()
    assert LlavaHipEngine.kv_next_positions(MASK, 6).tolist() == [3, 6, 5]


def caches(engine_cls, fanout=1):
    """the caches engine.new_kv_cache / new_shared_kv_cache make, on the host (no allocation of K / V)"""
    eng = SimpleNamespace(L=2, nkv=1, hd=128, dev=torch.device("cpu"), kv_next_positions=engine_cls.kv_next_positions)
    if fanout == 1:
        return engine_cls.new_kv_cache(eng, MASK.shape[0], 4)
    return engine_cls.new_shared_kv_cache(eng, MASK.shape[0], fanout, 4)


def test_caches_start_at_the_engines_positions():
    from vlrlhf.engine import KVCache, LlavaHipEngine
    from vlrlhf.engine_qwen import QwenVLHipEngine
    S = MASK.shape[1]
    for cls, first in ((QwenVLHipEngine, [8, 8, 8]), (LlavaHipEngine, [5, 8, 7])):
        c = caches(cls)
        c.reserve(S, alloc=False)
        c.start(MASK)
        assert c.pos.dtype == torch.int32 and c.pos.tolist() == first and c.len == S
        c.open_column()
        c.advance()
        assert c.pos.tolist() == [p + 1 for p in first] and c.len == S + 1
        sh = caches(cls, fanout=2)
        sh.prompt.reserve(S, alloc=False)
        sh.prompt.start(MASK)
        sh.begin(alloc=False)
        assert sh.pos.tolist() == [p for p in first for _ in range(2)], "every sample starts where its prompt's next token sits"
        sh.open_column()
        sh.advance()
        assert sh.pos.tolist() == [p + 1 for p in first for _ in range(2)]
    bare = KVCache(2, 3, 1, 128, 4, "cpu")                      # a cache made by hand keeps the merge's rule
    bare.reserve(S, alloc=False)
    bare.start(MASK)
    assert bare.position_rule is None and bare.pos.tolist() == [5, 8, 7]


def test_enable_kv_cache_touches_the_instance_only():
    from vlrlhf.engine import LlavaHipEngine
    from vlrlhf.engine_qwen import QwenVLHipEngine
    from vlrlhf.models.QwenVL import QwenVLForRL
    assert QwenVLHipEngine.supports_kv_cache is False and LlavaHipEngine.supports_kv_cache is True
    eng, other = object.__new__(QwenVLHipEngine), object.__new__(QwenVLHipEngine)      # (no GPU: the constructor is not run)
    model = SimpleNamespace(engine=eng)
    assert not eng.supports_kv_cache
    assert QwenVLForRL.enable_kv_cache(model) is model
    assert eng.supports_kv_cache is True and "supports_kv_cache" in vars(eng)
    assert QwenVLHipEngine.supports_kv_cache is False and not other.supports_kv_cache, "the class and every other engine stay on the loop"
    QwenVLForRL.enable_kv_cache(model, False)
    assert eng.supports_kv_cache is False
    assert QwenVLForRL.text_only_prompts and not hasattr(QwenVLForRL.__mro__[1], "text_only_prompts")


def test_cached_prefill_resolves_the_pixels_once(monkeypatch):
    """the images ride in the ids: without pixel_values the cached route looks the files up from the PROMPT ids, once"""
    import vlrlhf.models.QwenVL as Q
    seen = {}
    monkeypatch.setattr(Q.LlavaForRL, "_generate_cached", lambda self, ids, *a, **k: seen.update(img=a[9], kw=k) or ids)
    looked = []
    me = SimpleNamespace(_pixels_from_ids=lambda ids: looked.append(ids) or "pixels")
    ids = torch.zeros(2, 3, dtype=torch.long)
    rest = (None, 5, False, 1.0, 50, 1.0, 0, {2}, None)
    Q.QwenVLForRL._generate_cached(me, ids, *rest, {"pixel_values": None}, "plain", fanout=3)
    assert seen["img"] == {"pixel_values": "pixels"} and len(looked) == 1 and looked[0] is ids and seen["kw"] == {"fanout": 3}
    Q.QwenVLForRL._generate_cached(me, ids, *rest, {"pixel_values": "given"}, "plain")
    assert seen["img"] == {"pixel_values": "given"} and len(looked) == 1
