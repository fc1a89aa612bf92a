"""generate() and engine.decode_step with LIVE LoRA adapters on the MI355X: nothing merged, nothing cloned - the prefill applies the
adapters as every training forward does and each decode step runs vlr_decoder_layer_decode_lora (bf16 base) or _w4_lora (packed GPTQ
base, into which nothing can be merged).  LLaVA-1.5 (llava_hipsmall) and LLaVA-Next-Mistral (llavanext_small, grouped-query) at r = 8
with random non-zero lora_B.  Needs a real MI355X:  pytest -m gpu"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gptq_ref as R  # noqa: E402
from tests.golden_util import load_case  # noqa: E402

PEFT = dict(r=8, lora_alpha=16, lora_dropout=0.0, target_modules="auto", bias="none")


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


def wake_adapters(model):
    g = torch.Generator().manual_seed(5)
    for v in model.engine.lv.values():                       # non-zero lora_B: the adapters change every projection
        v.copy_((torch.randn(v.shape, generator=g) * 0.05).to(v.dtype))


def llava(name, lora=True, r=8):
    z, cfg, W, W_ref, batch, rows = load_case(name)
    if name == "llavanext_small":
        from vlrlhf.models.LlavaNext import LlavaNextForRL as Cls
    else:
        from vlrlhf.models.Llava import LlavaForRL as Cls
    model = Cls.from_state_dict(cfg, W)
    if lora:
        model.apply_lora(dict(PEFT, r=r))
        wake_adapters(model)
    model.eval()
    return cfg, W, batch, model


def prompt_kw(batch, gpu):
    img = {k: v.to(gpu) for k, v in batch["img_input_dict"].items()}
    return dict(input_ids=batch["prompt_input_ids"].to(gpu), attention_mask=batch["prompt_attention_mask"].to(gpu), **img)


class Spy:
    """counts engine.forward_hidden calls (and the weight set each one ran on), records the lm-head logits of every step (the
    vlr_gemm_bf16 lm-head call of the prefill / re-forward loop, the logits engine.decode_step returns) and every entry point called"""

    def __init__(self, model, monkeypatch):
        from vlrlhf import _hip
        import vlrlhf.engine as E
        import vlrlhf.models.Llava as LL
        eng = model.engine
        self.calls, self.ws, self.logits, self.steps, self.names = 0, [], [], 0, []
        fh, ds, call = eng.forward_hidden, eng.decode_step, _hip.call
        lm_ids = {id(model.weights.v["lm_head"])}

        def forward_hidden(ws, *a, **k):
            self.calls += 1
            self.ws.append(ws)
            lm_ids.add(id(ws.v["lm_head"]))
            return fh(ws, *a, **k)

        def decode_step(*a, **k):
            self.steps += 1
            out = ds(*a, **k)
            self.logits.append(out.clone())
            return out

        def spy_call(name, *args):
            self.names.append(name)
            rc = call(name, *args)
            if name == "vlr_gemm_bf16" and id(args[2]) in lm_ids:
                self.logits.append(args[3].clone())
            return rc

        monkeypatch.setattr(eng, "forward_hidden", forward_hidden)
        monkeypatch.setattr(eng, "decode_step", decode_step)
        assert LL._hip is _hip and E._hip is _hip
        monkeypatch.setattr(_hip, "call", spy_call)


def padded_prompt(batch, gpu):
    ids, mask = batch["prompt_input_ids"].to(gpu), batch["prompt_attention_mask"].to(gpu)
    Bn, T = ids.shape
    Tp = (T + 31) // 32 * 32
    fill = torch.zeros(Bn, Tp - T, dtype=ids.dtype, device=gpu)
    return torch.cat([fill, ids], 1), torch.cat([torch.zeros_like(fill), mask], 1)


@pytest.mark.parametrize("name", ["llava_hipsmall", "llavanext_small"])
def test_generate_unmerged_runs_live_adapters(gpu, name, monkeypatch):
    """merge_lora=False: ONE prefill, on the policy itself; merged_weights is never called; the first token's logits are those of the
    re-forward loop bit for bit; later steps within bf16 tolerance of it on an identical prefix (the bound and rule of
    test_cached_generate_matches_reforward_loop); the first two tokens agree"""
    cfg, W, batch, model = llava(name)
    eng = model.engine
    new = 5
    kw = dict(prompt_kw(batch, gpu), max_new_tokens=new, do_sample=False, pad_token_id=0, eos_token_id=10 ** 6)
    B = kw["input_ids"].shape[0]
    s_ref = Spy(model, monkeypatch)
    out_ref = model.generate(use_cache=False, **kw)
    assert s_ref.calls == new
    monkeypatch.undo()
    monkeypatch.setattr(eng, "merged_weights", lambda *a, **k: pytest.fail("merge_lora=False cloned and merged the policy"))
    s = Spy(model, monkeypatch)
    out = model.generate(merge_lora=False, **kw)
    assert s.calls == 1 and s.ws[0] is eng.policy, "one prefill, on the policy with its adapters live"
    assert s.steps == new - 1
    assert s.names.count("vlr_decoder_layer_decode_lora") == (new - 1) * eng.L and "vlr_decoder_layer_decode" not in s.names
    assert len(s.logits) == len(s_ref.logits) == new
    assert torch.equal(s.logits[0][:B], s_ref.logits[0][:B]), "first step: same prefill, same lm-head call"
    T0 = kw["input_ids"].shape[1]
    for k in range(1, new):
        if not torch.equal(out[:, :T0 + k], out_ref[:, :T0 + k]):
            break                                              # (a bf16 near-tie changed the prefix: nothing left to compare)
        e = relerr(s.logits[k][:B], s_ref.logits[k][:B])
        print(f"{name} step {k}: live decode vs re-forward loop rel err {e:.3e} (bound 2e-2)")
        assert e < 2e-2, (k, e)
    assert torch.equal(out[:, :T0 + 2], out_ref[:, :T0 + 2])


def test_generate_unmerged_at_rank_256(gpu, monkeypatch):
    """r = 256 on q | k | v (3 r = 768 columns of u): the live path takes any rank the training path takes - one prefill on the policy,
    live decode steps, first logits those of the re-forward loop bit for bit, the next step within the bf16 bound"""
    cfg, W, batch, model = llava("llava_hipsmall", r=256)
    eng = model.engine
    kw = dict(prompt_kw(batch, gpu), max_new_tokens=2, do_sample=False, pad_token_id=0, eos_token_id=10 ** 6)
    B = kw["input_ids"].shape[0]
    s_ref = Spy(model, monkeypatch)
    out_ref = model.generate(use_cache=False, **kw)
    monkeypatch.undo()
    monkeypatch.setattr(eng, "merged_weights", lambda *a, **k: pytest.fail("merge_lora=False cloned and merged the policy"))
    s = Spy(model, monkeypatch)
    out = model.generate(merge_lora=False, **kw)
    assert s.calls == 1 and s.ws[0] is eng.policy and s.names.count("vlr_decoder_layer_decode_lora") == eng.L
    assert torch.equal(s.logits[0][:B], s_ref.logits[0][:B])
    assert torch.equal(out[:, :-1], out_ref[:, :-1])
    e = relerr(s.logits[1][:B], s_ref.logits[1][:B])
    print(f"r = 256 step 1: live decode vs re-forward loop rel err {e:.3e} (bound 2e-2)")
    assert e < 2e-2, e


@pytest.mark.parametrize("name", ["llava_hipsmall", "llavanext_small"])
def test_live_decode_step_matches_merged_weights(gpu, name):
    """decode_step on (policy, live adapters) against (merged weights, no adapters) from the same cache contents: the existing
    merged-vs-unmerged bound"""
    cfg, W, batch, model = llava(name)
    eng = model.engine
    run_ids, run_mask = padded_prompt(batch, gpu)
    pv = batch["img_input_dict"]["pixel_values"].to(gpu)
    sizes = batch["img_input_dict"].get("image_sizes")
    sizes = sizes.to(gpu) if isinstance(sizes, torch.Tensor) else sizes
    Bn = run_ids.shape[0]
    with torch.no_grad():
        cache = eng.new_kv_cache(Bn, 4)
        c = eng.forward_hidden(eng.policy, run_ids, run_mask, None, pv, save=False, tag="policy_ng", image_sizes=sizes, kv_cache=cache)
        tok = model._last_logits(c, Bn, eng.policy.v["lm_head"]).argmax(-1)
        twin = eng.new_kv_cache(Bn, 4)                         # the same cache contents for the merged run
        eng.forward_hidden(eng.policy, run_ids, run_mask, None, pv, save=False, tag="policy_ng", image_sizes=sizes, kv_cache=twin)
        for l in range(eng.L):
            n = cache.len                                      # the filled columns
            assert twin.len == n and torch.equal(cache.k[l][:, :, :n], twin.k[l][:, :, :n]) and torch.equal(cache.v[l][:, :, :n], twin.v[l][:, :, :n])
        merged = eng.merged_weights()
        for k in range(3):
            live = eng.decode_step(eng.policy, tok, cache)
            ref = eng.decode_step(merged, tok, twin)
            torch.cuda.synchronize()
            e = relerr(live, ref)
            print(f"{name} step {k}: live vs merged rel err {e:.3e} (bound 2e-2)")
            assert torch.isfinite(live).all() and e < 2e-2, (k, e)
            tok = ref.argmax(-1)
        with model.disable_adapter():                          # the adapters matter: the base weights alone are further away
            off = eng.decode_step(eng.policy, tok, cache)
        assert relerr(off, eng.decode_step(merged, tok, twin)) > e


def test_disabled_adapters_make_todays_calls(gpu, monkeypatch):
    """disable_adapter(): decode_step reaches no _lora entry point and its logits equal those of a model without LoRA, bit for bit"""
    cfg, W, batch, model = llava("llava_hipsmall")
    _, _, _, bare = llava("llava_hipsmall", lora=False)
    run_ids, run_mask = padded_prompt(batch, gpu)
    pv = batch["img_input_dict"]["pixel_values"].to(gpu)
    Bn = run_ids.shape[0]
    outs = []
    for m in (model, bare):
        eng = m.engine
        s = Spy(m, monkeypatch)
        with torch.no_grad(), m.disable_adapter():
            cache = eng.new_kv_cache(Bn, 3)
            c = eng.forward_hidden(eng.policy, run_ids, run_mask, None, pv, save=False, tag="policy_ng", kv_cache=cache)
            tok = m._last_logits(c, Bn, eng.policy.v["lm_head"]).argmax(-1)
            outs.append([eng.decode_step(eng.policy, tok, cache).clone(), eng.decode_step(eng.policy, tok, cache).clone()])
        torch.cuda.synchronize()
        assert not [n for n in s.names if n.endswith("_lora")], "an adapter entry point with the adapters disabled"
        assert s.names.count("vlr_decoder_layer_decode") == 2 * eng.L
        monkeypatch.undo()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    with pytest.raises(ValueError, match="live adapters"):
        with model.disable_adapter():
            model.engine.decode_step(model.engine.policy, tok, cache, lora=True)


def test_packed_base_decodes_with_live_adapters(gpu, tmp_path, monkeypatch):
    """GPTQ int4 base + active adapters: generate takes the cached path (ONE forward_hidden, then decode steps on the packed weights
    with the adapters live), whatever merge_lora says; its logits stay within bf16 tolerance of the bf16-dequantised twin running
    merge_lora=False"""
    from vlrlhf.models.Llava import LlavaForRL, _hf_from_cfg
    z, cfg, W, W_ref, batch, rows = load_case("llava_hipsmall")
    deq = R.write_checkpoint(str(tmp_path), _hf_from_cfg(cfg), W, 32)
    A = LlavaForRL.from_pretrained(str(tmp_path))
    B = LlavaForRL.from_state_dict({k: v for k, v in A.engine.cfg.items() if k != "gptq"}, deq)
    assert A.is_packed and not B.is_packed
    for m in (A, B):
        m.apply_lora(dict(PEFT))
        wake_adapters(m)
        m.eval()
    new = 4
    kw = dict(prompt_kw(batch, gpu), max_new_tokens=new, do_sample=False, pad_token_id=0, eos_token_id=10 ** 6)
    Bn = kw["input_ids"].shape[0]
    sa = Spy(A, monkeypatch)
    out_a = A.generate(**kw)                                   # default merge_lora: nothing to merge into packed weights
    assert sa.calls == 1 and sa.ws[0] is A.engine.policy, "the packed model with active adapters decodes from the cache"
    assert sa.steps == new - 1
    assert sa.names.count("vlr_decoder_layer_decode_w4_lora") == (new - 1) * A.engine.L
    assert "vlr_decoder_layer_decode_w4" not in sa.names and "vlr_decoder_layer_decode_lora" not in sa.names
    monkeypatch.undo()
    sb = Spy(B, monkeypatch)
    out_b = B.generate(merge_lora=False, **kw)
    assert sb.calls == 1 and sb.names.count("vlr_decoder_layer_decode_lora") == (new - 1) * B.engine.L
    assert len(sa.logits) == len(sb.logits) == new
    T0 = kw["input_ids"].shape[1]
    for k in range(new):
        if not torch.equal(out_a[:, :T0 + k], out_b[:, :T0 + k]):
            break                                              # (a near-tie changed the prefix: nothing left to compare)
        e = relerr(sa.logits[k][:Bn], sb.logits[k][:Bn])
        print(f"step {k}: packed + live adapters vs bf16 twin rel err {e:.3e} (bound 2e-2)")
        assert e < 2e-2, (k, e)
    assert torch.equal(out_a[:, :T0 + 1], out_b[:, :T0 + 1])
