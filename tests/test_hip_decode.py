"""generate(use_cache=True) end to end on the MI355X: one prefill into the KV cache, then one decode step per token, on LLaVA-1.5
(llava_hipsmall) and LLaVA-Next-Mistral (llavanext_small, grouped-query); the re-forward loop (use_cache=False) and the fp32 oracle
are the yardsticks.  Qwen-VL and InternLM-XComposer2 keep the re-forward loop.  Needs a real MI355X:  pytest -m gpu"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import llava_dpo_oracle as O  # noqa: E402  (checker only)
from tests.golden_util import load_case  # noqa: E402


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return torch.device("cuda")


def relerr(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-12)


def llava(name):
    z, cfg, W, W_ref, batch, rows = load_case(name)
    if name == "llavanext_small":
        from vlrlhf.models.LlavaNext import LlavaNextForRL as Cls
    else:
        from vlrlhf.models.Llava import LlavaForRL as Cls
    model = Cls.from_state_dict(cfg, W)
    return cfg, W, batch, model


def prompt_kw(batch, gpu):
    img = {k: v.to(gpu) for k, v in batch["img_input_dict"].items()}
    return dict(input_ids=batch["prompt_input_ids"].to(gpu), attention_mask=batch["prompt_attention_mask"].to(gpu), **img)


class Spy:
    """counts engine.forward_hidden calls (and the weight set each one ran on) and records the lm-head logits of every step:
    the vlr_gemm_bf16 lm-head call of the prefill / re-forward loop and the logits engine.decode_step returns"""

    def __init__(self, model, monkeypatch):
        from vlrlhf import _hip
        import vlrlhf.models.Llava as LL
        eng = model.engine
        self.calls, self.ws, self.logits = 0, [], []
        fh, ds, call = eng.forward_hidden, eng.decode_step, _hip.call
        lm_ids = {id(model.weights.v["lm_head"])}

        def forward_hidden(ws, *a, **k):
            self.calls += 1
            self.ws.append(ws)
            lm_ids.add(id(ws.v["lm_head"]))
            return fh(ws, *a, **k)

        def decode_step(*a, **k):
            out = ds(*a, **k)
            self.logits.append(out.clone())
            return out

        def spy_call(name, *args):
            rc = call(name, *args)
            if name == "vlr_gemm_bf16" and id(args[2]) in lm_ids:
                self.logits.append(args[3].clone())
            return rc

        monkeypatch.setattr(eng, "forward_hidden", forward_hidden)
        monkeypatch.setattr(eng, "decode_step", decode_step)
        monkeypatch.setattr(LL._hip, "call", spy_call)


@pytest.mark.parametrize("name", ["llava_hipsmall", "llavanext_small"])
def test_cached_generate_matches_reforward_loop(gpu, name, monkeypatch):
    """one prefill per cached generate; the first token's logits are bit-identical to use_cache=False, later steps match the
    re-forward loop's logits on the same prefix within bf16 tolerance; the tokens agree"""
    cfg, W, batch, model = llava(name)
    assert model.engine.supports_kv_cache
    kw = dict(prompt_kw(batch, gpu), max_new_tokens=6, do_sample=False, pad_token_id=0, eos_token_id=10 ** 6)
    B = kw["input_ids"].shape[0]
    s_ref = Spy(model, monkeypatch)
    out_ref = model.generate(use_cache=False, **kw)
    assert s_ref.calls == 6
    monkeypatch.undo()
    s = Spy(model, monkeypatch)
    out = model.generate(**kw)                                 # use_cache defaults to True
    assert s.calls == 1, "the cached path runs ONE prefill"
    assert len(s.logits) == len(s_ref.logits) == 6
    assert torch.equal(s.logits[0][:B], s_ref.logits[0][:B]), "first step: same prefill, same lm-head call"
    T0 = kw["input_ids"].shape[1]
    for k in range(1, 6):
        if not torch.equal(out[:, :T0 + k], out_ref[:, :T0 + k]):
            break                                              # (a bf16 near-tie changed the prefix: nothing left to compare)
        e = relerr(s.logits[k][:B], s_ref.logits[k][:B])
        assert e < 2e-2, (k, e)
    assert torch.equal(out[:, :T0 + 2], out_ref[:, :T0 + 2])


def test_cached_greedy_tokens_against_oracle(gpu):
    """greedy tokens of the cached path judged against the fp32 oracle's teacher-forced next-token logits (the rule of
    test_generate_and_get_batch_samples); sampling under a generator is reproducible; eos rows receive the pad id afterwards"""
    cfg, W, batch, model = llava("llava_hipsmall")
    pix = batch["img_input_dict"]["pixel_values"]
    ids0, m0 = batch["prompt_input_ids"], batch["prompt_attention_mask"]
    new = 6
    out = model.generate(input_ids=ids0.to(gpu), attention_mask=m0.to(gpu), max_new_tokens=new, do_sample=False, pad_token_id=0,
                         eos_token_id=10 ** 6, pixel_values=pix.to(gpu), use_cache=True).cpu()
    assert out.shape == (2, ids0.shape[1] + new) and torch.equal(out[:, :ids0.shape[1]], ids0)
    ids, mask = ids0.clone(), m0.clone()
    for k in range(new):
        logits, _, aux = O.llava_forward(W, cfg, ids, mask, torch.full_like(ids, -100), pix, dedupe_images=False)
        for b in range(2):
            last = int(torch.nonzero(aux["mask"][b]).max())
            row = logits[b, last]
            tok = int(out[b, ids0.shape[1] + k])
            assert float(row.max() - row[tok]) <= 0.06 * float(row.max() - row.min()), (k, b, tok, int(row.argmax()))
        ids = torch.cat([ids, out[:, ids0.shape[1] + k: ids0.shape[1] + k + 1]], 1)
        mask = torch.cat([mask, torch.ones(2, 1, dtype=mask.dtype)], 1)
    g = lambda: torch.Generator(device=gpu).manual_seed(11)      # noqa: E731
    kw = dict(input_ids=ids0.to(gpu), attention_mask=m0.to(gpu), max_length=ids0.shape[1] + 5, do_sample=True, top_k=5, pad_token_id=0,
              eos_token_id=10 ** 6, pixel_values=pix.to(gpu))
    s1, s2 = model.generate(generator=g(), **kw).cpu(), model.generate(generator=g(), **kw).cpu()
    assert torch.equal(s1, s2) and s1.shape[1] == ids0.shape[1] + 5
    first = int(out[0, ids0.shape[1]])
    e = model.generate(input_ids=ids0.to(gpu), attention_mask=m0.to(gpu), max_new_tokens=5, do_sample=False, pad_token_id=191,
                       eos_token_id=first, pixel_values=pix.to(gpu)).cpu()
    assert int(e[0, ids0.shape[1]]) == first and bool((e[0, ids0.shape[1] + 1:] == 191).all())


def test_cached_generate_with_lora_policy_and_disabled_adapters(gpu, monkeypatch):
    """LoRA-active policy: one prefill on the merged weights (not the policy's base weights); adapters disabled (trl's null_ref_context):
    one prefill on the base weights - both on the cached path, both close to the re-forward loop on the same weights"""
    cfg, W, batch, model = llava("llava_hipsmall")
    model.apply_lora(dict(r=8, lora_alpha=16, lora_dropout=0.0, target_modules="auto", bias="none"))
    g = torch.Generator().manual_seed(5)
    for v in model.engine.lv.values():                       # non-zero lora_B: the merge changes the weights
        v.copy_((torch.randn(v.shape, generator=g) * 0.05).to(v.dtype))
    model.eval()
    kw = dict(prompt_kw(batch, gpu), max_new_tokens=3, do_sample=False, pad_token_id=0, eos_token_id=10 ** 6)
    B = kw["input_ids"].shape[0]
    s_ref = Spy(model, monkeypatch)
    model.generate(use_cache=False, **kw)
    monkeypatch.undo()
    s = Spy(model, monkeypatch)
    model.generate(**kw)
    assert s.calls == 1 and s.ws[0] is not model.engine.policy
    assert relerr(s.logits[0][:B], s_ref.logits[0][:B]) < 2e-2          # merged (cached) vs un-merged adapters (re-forward loop)
    monkeypatch.undo()
    with model.disable_adapter():
        s_ref = Spy(model, monkeypatch)
        model.generate(use_cache=False, **kw)
        monkeypatch.undo()
        s = Spy(model, monkeypatch)
        model.generate(**kw)
    assert s.calls == 1 and s.ws[0] is model.engine.policy
    assert torch.equal(s.logits[0][:B], s_ref.logits[0][:B])


@pytest.mark.parametrize("family", ["qwenvl", "internlm"])
def test_models_without_cache_still_generate(gpu, family, monkeypatch):
    """Qwen-VL and InternLM-XComposer2 have no KV-cache path (supports_kv_cache False): generate re-runs the forward per token and
    never reaches decode_step.  (Qwen-VL: one new token - a random model may emit an image marker, which its merge rejects on the
    next re-forward: a property of its text-embedded image ids, not of the cache.)"""
    if family == "qwenvl":
        from vlrlhf.models.QwenVL import QwenVLForRL as Cls
        z, cfg, W, W_ref, batch, _ = load_case("qwenvl_small")
        new = 1
    else:
        from vlrlhf.models.InternLMXC2 import InternLMXC2ForRL as Cls
        z, cfg, W, W_ref, batch, _ = load_case("internlmxc2_small")
        new = 3
    model = Cls.from_state_dict(cfg, W)
    assert not model.engine.supports_kv_cache
    ids, m = batch["chosen_input_ids"].to(gpu), batch["chosen_attention_mask"].to(gpu)
    calls = []
    fh = model.engine.forward_hidden
    monkeypatch.setattr(model.engine, "forward_hidden", lambda *a, **k: (calls.append(1), fh(*a, **k))[1])
    monkeypatch.setattr(model.engine, "decode_step", lambda *a, **k: pytest.fail("decode_step on an engine without a KV cache"))
    out = model.generate(input_ids=ids, attention_mask=m, max_new_tokens=new, do_sample=False, pad_token_id=0, eos_token_id=10 ** 6,
                         pixel_values=batch["img_input_dict"]["pixel_values"].to(gpu))
    assert out.shape == (ids.shape[0], ids.shape[1] + new) and torch.equal(out[:, :ids.shape[1]].cpu(), ids.cpu())
    assert len(calls) == new
