"""generate(num_return_sequences=n) end to end on the MI355X: one prefill of the P prompts into a SharedPromptKVCache, then one decode
step per token for the P * n samples over the shared prompt K / V, on LLaVA-1.5 (llava_hipsmall) and LLaVA-Next-Mistral
(llavanext_small, grouped-query).  The yardstick is the existing cached route on the repeat_interleave-expanded batch, teacher-forced
with the same tokens.  Needs a real MI355X:  pytest -m gpu"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.golden_util import load_case  # noqa: E402
from tests.test_hip_decode import Spy, llava, prompt_kw, relerr  # noqa: E402


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return torch.device("cuda")


def gen(gpu, seed=11):
    return torch.Generator(device=gpu).manual_seed(seed)


def expanded(model, kw, n):
    """the batch of `kw` with every prompt repeated n times, in repeat_interleave order"""
    B = kw["input_ids"].shape[0]
    return {k: model._expand_rows(v, B, n) for k, v in kw.items()}


@pytest.mark.parametrize("name", ["llava_hipsmall", "llavanext_small"])
def test_generate_num_return_sequences(gpu, name, monkeypatch):
    """shape, row order, diversity, one prefill, every layer of every step through the shared entry point, EOS padding"""
    from vlrlhf import _hip
    import vlrlhf.engine as E
    cfg, W, batch, model = llava(name)
    kw = dict(prompt_kw(batch, gpu), do_sample=True, pad_token_id=0, eos_token_id=10 ** 6)
    ids0 = kw["input_ids"]
    P, T = ids0.shape
    names = []
    call = _hip.call
    monkeypatch.setattr(E._hip, "call", lambda nm, *a: (names.append(nm), call(nm, *a))[1])
    s = Spy(model, monkeypatch)
    out = model.generate(num_return_sequences=3, max_new_tokens=6, generator=gen(gpu), **kw)
    monkeypatch.undo()
    assert s.calls == 1, "one prefill for the P prompts"
    assert names.count("vlr_decoder_layer_decode_shared") == 5 * model.engine.L and "vlr_decoder_layer_decode" not in names
    assert out.shape == (P * 3, T + 6)
    for p in range(P):
        assert torch.equal(out[3 * p:3 * p + 3, :T], ids0[p].expand(3, T)), "rows 3p .. 3p+2 carry prompt p"
    assert any(not (torch.equal(out[3 * p], out[3 * p + 1]) and torch.equal(out[3 * p], out[3 * p + 2])) for p in range(P)), \
        "the samples of at least one prompt differ"
    out2 = model.generate(num_return_sequences=3, max_new_tokens=6, generator=gen(gpu), **kw)
    assert torch.equal(out, out2), "same seed, same samples"
    # EOS: the first token of row 0 as the eos id -> that row is padded from then on, and so is every row that drew it
    first = int(out[0, T])
    e = model.generate(num_return_sequences=3, max_new_tokens=6, generator=gen(gpu), **dict(kw, eos_token_id=first, pad_token_id=191))
    assert e.shape[0] == P * 3 and T < e.shape[1] <= T + 6
    assert int(e[0, T]) == first
    for row in e[:, T:]:
        hit = (row == first).nonzero()
        if len(hit):
            assert bool((row[int(hit[0]) + 1:] == 191).all()), "finished rows receive the pad id"


def teacher_forced_parity(model, kw, gpu, monkeypatch, n=3, new=6, **extra):
    """per-step logits of the shared route against the existing cached route on the expanded batch fed the SAME tokens -> worst
    relative error (every step, the first included, under the bound of test_cached_generate_matches_reforward_loop: 2e-2)"""
    B = kw["input_ids"].shape[0]
    s = Spy(model, monkeypatch)
    out = model.generate(num_return_sequences=n, max_new_tokens=new, generator=gen(gpu), **kw, **extra)
    monkeypatch.undo()
    assert s.calls == 1 and len(s.logits) == new
    T = kw["input_ids"].shape[1]
    toks = [out[:, T + k] for k in range(new)]
    step = [0]

    def forced(probs, num, generator=None):
        k = step[0]
        step[0] += 1
        return toks[k][:, None].clone()

    s_ref = Spy(model, monkeypatch)
    monkeypatch.setattr(torch, "multinomial", forced)
    out_ref = model.generate(max_new_tokens=new, generator=gen(gpu), **expanded(model, kw, n), **extra)
    monkeypatch.undo()
    assert torch.equal(out_ref, out) and len(s_ref.logits) == new
    worst = 0.0
    for k in range(new):
        a = s.logits[k][:B].repeat_interleave(n, 0) if k == 0 else s.logits[k]
        e = relerr(a, s_ref.logits[k][:B * n])
        print(f"  step {k}: shared vs expanded-batch logits, relative error {e:.3e}")
        assert e < 2e-2, (k, e)
        worst = max(worst, e)
    return worst


@pytest.mark.parametrize("name", ["llava_hipsmall", "llavanext_small"])
def test_shared_route_matches_expanded_batch_teacher_forced(gpu, name, monkeypatch):
    cfg, W, batch, model = llava(name)
    kw = dict(prompt_kw(batch, gpu), do_sample=True, pad_token_id=0, eos_token_id=10 ** 6)
    teacher_forced_parity(model, kw, gpu, monkeypatch)


def test_live_adapters_take_the_shared_route(gpu, monkeypatch):
    """merge_lora=False with active adapters: nothing merged, the shared route agrees with its expanded-batch counterpart"""
    cfg, W, batch, model = llava("llava_hipsmall")
    model.apply_lora(dict(r=8, lora_alpha=16, lora_dropout=0.0, target_modules="auto", bias="none"))
    g = torch.Generator().manual_seed(5)
    for v in model.engine.lv.values():                       # non-zero lora_B: the adapters change the logits
        v.copy_((torch.randn(v.shape, generator=g) * 0.05).to(v.dtype))
    model.eval()
    assert model.cached_lora_route(False) == "live"
    merged = []
    monkeypatch.setattr(model.engine, "merged_weights", lambda *a, **k: merged.append(1) or pytest.fail("merge_lora=False merged"))
    kw = dict(prompt_kw(batch, gpu), do_sample=True, pad_token_id=0, eos_token_id=10 ** 6)
    teacher_forced_parity(model, kw, gpu, monkeypatch, new=4, merge_lora=False)
    assert not merged


def test_routes(gpu, monkeypatch):
    cfg, W, batch, model = llava("llava_hipsmall")
    kw = dict(prompt_kw(batch, gpu), max_new_tokens=4, pad_token_id=0, eos_token_id=10 ** 6)
    P, T = kw["input_ids"].shape
    # n == 1: what the call without the keyword returns
    a = model.generate(do_sample=True, generator=gen(gpu), **kw)
    b = model.generate(do_sample=True, generator=gen(gpu), num_return_sequences=1, **kw)
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="num_return_sequences"):
        model.generate(do_sample=False, num_return_sequences=2, **kw)
    # use_cache=False: the expansion, never the decode step
    monkeypatch.setattr(model.engine, "decode_step", lambda *a, **k: pytest.fail("decode_step under use_cache=False"))
    o = model.generate(do_sample=True, generator=gen(gpu), num_return_sequences=2, use_cache=False, **kw)
    monkeypatch.undo()
    assert o.shape == (P * 2, T + 4)
    for p in range(P):
        assert torch.equal(o[2 * p:2 * p + 2, :T], kw["input_ids"][p].expand(2, T))


def test_engine_without_cache_expands(gpu, monkeypatch):
    """InternLM-XComposer2 has no KV cache: num_return_sequences goes through the repeat_interleave expansion"""
    from vlrlhf.models.InternLMXC2 import InternLMXC2ForRL as Cls
    z, cfg, W, W_ref, batch, _ = load_case("internlmxc2_small")
    model = Cls.from_state_dict(cfg, W)
    assert not model.engine.supports_kv_cache
    ids, m = batch["chosen_input_ids"].to(gpu), batch["chosen_attention_mask"].to(gpu)
    monkeypatch.setattr(model.engine, "decode_step", lambda *a, **k: pytest.fail("decode_step on an engine without a KV cache"))
    out = model.generate(input_ids=ids, attention_mask=m, max_new_tokens=2, do_sample=True, generator=gen(gpu), num_return_sequences=2,
                         pad_token_id=0, eos_token_id=10 ** 6, pixel_values=batch["img_input_dict"]["pixel_values"].to(gpu))
    P, T = ids.shape
    assert out.shape == (P * 2, T + 2)
    for p in range(P):
        assert torch.equal(out[2 * p:2 * p + 2, :T], ids[p].expand(2, T))
