"""CPU-only checks of InternLM-XComposer2's opt-in KV cache: enable_kv_cache() touches one engine instance and leaves the class on the
re-forward loop; the rotary position of the first decoded token is the index in the merged sequence - `length` for every row, however
far it was left-padded - and reaches KVCache.start and SharedPromptKVCache.begin through the caches the engine makes; the layers
composed from bf16 primitives (VLR_ILM_LORA_FUSED=0) keep the loop, decided when generate starts."""
from types import SimpleNamespace

import pytest
import torch

MASK = torch.tensor([[0, 0, 0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 1, 1], [0, 1, 1, 1, 1, 1, 1, 1]], dtype=torch.int32)      # left-padded


def test_enable_kv_cache_touches_the_instance_only():
    from vlrlhf.engine_internlm import InternLMHipEngine
    from vlrlhf.models.InternLMXC2 import InternLMXC2ForRL
    assert InternLMHipEngine.supports_kv_cache is False
    eng, other = object.__new__(InternLMHipEngine), object.__new__(InternLMHipEngine)      # (no GPU: the constructor is not run)
    model = SimpleNamespace(engine=eng)
    assert not eng.supports_kv_cache
    assert InternLMXC2ForRL.enable_kv_cache(model) is model
    assert eng.supports_kv_cache is True and "supports_kv_cache" in vars(eng)
    assert InternLMHipEngine.supports_kv_cache is False and not other.supports_kv_cache, "the class and every other engine stay on the loop"
    InternLMXC2ForRL.enable_kv_cache(model, False)
    assert eng.supports_kv_cache is False and InternLMHipEngine.supports_kv_cache is False


def test_left_padded_rows_decode_at_the_merged_length():
    from vlrlhf.engine import KVCache, LlavaHipEngine
    from vlrlhf.engine_internlm import InternLMHipEngine
    S = MASK.shape[1]
    p = InternLMHipEngine.kv_next_positions(MASK, S)
    assert p.dtype == torch.int32 and p.tolist() == [S, S, S], "pos = arange(S) in every row: the next token sits at index S"
    assert InternLMHipEngine.kv_next_positions(MASK, 6).tolist() == [6, 6, 6] and InternLMHipEngine.kv_next_positions(MASK).tolist() == [S] * 3
    assert LlavaHipEngine.kv_next_positions(MASK, S).tolist() == [5, 8, 7] == KVCache.next_positions(MASK, S).tolist(), "LLaVA keeps the merge's rule"
    eng = SimpleNamespace(L=2, nkv=1, hd=128, dev=torch.device("cpu"), kv_next_positions=InternLMHipEngine.kv_next_positions)
    c = InternLMHipEngine.new_kv_cache(eng, MASK.shape[0], 4)
    c.reserve(S, alloc=False)
    c.start(MASK)
    assert c.pos.dtype == torch.int32 and c.pos.tolist() == [S, S, S] and c.len == S
    c.open_column()
    c.advance()
    assert c.pos.tolist() == [S + 1] * 3 and c.len == S + 1
    sh = InternLMHipEngine.new_shared_kv_cache(eng, MASK.shape[0], 2, 4)
    sh.prompt.reserve(S, alloc=False)
    sh.prompt.start(MASK)
    sh.begin(alloc=False)
    assert sh.pos.tolist() == [S] * 6, "every sample starts where its prompt's next token sits"
    sh.open_column()
    sh.advance()
    assert sh.pos.tolist() == [S + 1] * 6


def test_composed_layers_keep_the_loop_decided_at_generate_time(monkeypatch):
    import vlrlhf.models.InternLMXC2 as X
    from vlrlhf.engine import LlavaHipEngine
    from vlrlhf.engine_internlm import InternLMHipEngine
    eng = object.__new__(InternLMHipEngine)
    eng.lora, eng.lora_fused = None, False
    model = SimpleNamespace(engine=eng)
    seen = []
    monkeypatch.setattr(X.LlavaForRL, "generate", lambda self, *a, **k: seen.append((bool(self.engine.supports_kv_cache), a, k)) or "ids")
    assert X.InternLMXC2ForRL.generate(model, 1, use_cache=True) == "ids" and seen.pop() == (False, (1,), dict(use_cache=True)), "a fresh model: the loop"
    X.InternLMXC2ForRL.enable_kv_cache(model)
    assert eng.kv_cache_layers
    X.InternLMXC2ForRL.generate(model, 1, x=2)
    assert seen.pop() == (True, (1,), dict(x=2)), "full fine-tune weights: the cache, arguments passed through"
    # enable_lora AFTER the switch, composed layers (VLR_ILM_LORA_FUSED=0): the switch is withheld for the call and stands afterwards
    eng.lora, eng.lora_fused = dict(r=8), False
    assert not eng.kv_cache_layers and eng.supports_kv_cache
    X.InternLMXC2ForRL.generate(model, 1)
    assert seen.pop()[0] is False and eng.supports_kv_cache is True
    monkeypatch.setattr(X.LlavaForRL, "generate", lambda self, *a, **k: (_ for _ in ()).throw(RuntimeError("inside")))
    with pytest.raises(RuntimeError, match="inside"):
        X.InternLMXC2ForRL.generate(model, 1)
    assert eng.supports_kv_cache is True, "restored after an exception too"
    called = []
    monkeypatch.setattr(LlavaHipEngine, "decode_step", lambda self, *a: called.append(a) or "logits")
    with pytest.raises(ValueError, match="VLR_ILM_LORA_FUSED=0"):
        eng.decode_step(None, None, None)
    assert not called
    # the fused two-adapter layers (the default): the cache
    eng.lora_fused = True
    assert eng.kv_cache_layers and eng.decode_step("ws", "tok", "cache") == "logits" and called == [("ws", "tok", "cache", None)]
    monkeypatch.setattr(X.LlavaForRL, "generate", lambda self, *a, **k: seen.append(bool(self.engine.supports_kv_cache)) or "ids")
    X.InternLMXC2ForRL.generate(model, 1)
    assert seen.pop() is True
