"""Qwen-VL on the KV cache, switched on by the caller (QwenVLForRL.enable_kv_cache), end to end on the MI355X with the qwenvl_small
fixture.  The yardstick is the model's own re-forward loop (use_cache=False: what a fresh model does) fed the SAME tokens.  The loop
rejects a generated image-marker id on its next re-forward, so tokens are chosen by a stand-in for torch.multinomial that takes the
most likely id BELOW image_start_id (both routes run with do_sample=True and see the same stand-in); the cached route is then
teacher-forced on the loop's tokens.  Bounds are the existing ones: first-step logits bit for bit, later steps 2e-2 relative
(test_cached_generate_matches_reforward_loop).  Needs a real MI355X:  pytest -m gpu"""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.golden_util import load_case  # noqa: E402
from tests.test_hip_decode_lora import PEFT, Spy, relerr, wake_adapters  # noqa: E402
from tests.test_hip_decode_shared import teacher_forced_parity  # noqa: E402

PAD, NO_EOS = 510, 10 ** 6


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return torch.device("cuda")


def qwen(gpu, lora=False, repeat=1):
    """-> (cfg, model, kw): two prompts of 25 and 30 tokens (each with its image span), LEFT-padded to 30; repeat: the rows repeated"""
    from vlrlhf.models.QwenVL import QwenVLForRL
    z, cfg, W, W_ref, batch, _ = load_case("qwenvl_small")
    model = QwenVLForRL.from_state_dict(cfg, W)
    if lora:
        model.apply_lora(dict(PEFT, r=8))
        wake_adapters(model)
    model.eval()
    src, lens, T = batch["chosen_input_ids"], (25, 30), 30
    ids = torch.full((2, T), PAD, dtype=torch.long)
    mask = torch.zeros(2, T, dtype=torch.long)
    for i, n in enumerate(lens):
        ids[i, T - n:] = src[i, :n]
        mask[i, T - n:] = 1
    assert int((ids == cfg["image_start_id"]).sum()) == 2 and bool((mask[:, 0] == 0).any()) and int(mask[0].sum()) != int(mask[1].sum())
    px = batch["img_input_dict"]["pixel_values"]
    kw = dict(input_ids=ids.repeat(repeat, 1).to(gpu), attention_mask=mask.repeat(repeat, 1).to(gpu),
              pixel_values=px.repeat(repeat, 1, 1, 1).to(gpu), do_sample=True, pad_token_id=PAD, eos_token_id=NO_EOS)
    return cfg, model, kw


def below_markers(cfg):
    """stand-in for torch.multinomial: the most likely id below image_start_id (ids the re-forward loop can embed again)"""
    return lambda probs, num, generator=None: probs[:, :cfg["image_start_id"]].argmax(-1, keepdim=True)


def replay(out, T0):
    """stand-in for torch.multinomial: step k returns column T0 + k of `out` (teacher forcing)"""
    step = [0]

    def forced(probs, num, generator=None):
        step[0] += 1
        return out[:, T0 + step[0] - 1][:, None].clone()
    return forced


def loop_run(model, kw, cfg, monkeypatch, **extra):
    """the re-forward loop on restricted-greedy tokens -> (ids, spy)"""
    s = Spy(model, monkeypatch)
    monkeypatch.setattr(torch, "multinomial", below_markers(cfg))
    out = model.generate(use_cache=False, **kw, **extra)
    monkeypatch.undo()
    return out, s


def cached_run(model, kw, monkeypatch, pick, **extra):
    s = Spy(model, monkeypatch)
    monkeypatch.setattr(torch, "multinomial", pick)
    out = model.generate(use_cache=True, **kw, **extra)
    monkeypatch.undo()
    return out, s


def test_greedy_generation_matches_the_reforward_loop(gpu, monkeypatch):
    cfg, model, kw = qwen(gpu)
    eng, new = model.engine, 6
    B, T0 = kw["input_ids"].shape
    # a fresh model re-forwards, use_cache=True or not
    assert not eng.supports_kv_cache
    out0, s0 = cached_run(model, kw, monkeypatch, below_markers(cfg), max_new_tokens=2)
    assert s0.calls == 2 and s0.steps == 0, "a fresh model runs the re-forward loop"
    out_ref, s_ref = loop_run(model, kw, cfg, monkeypatch, max_new_tokens=new)
    assert s_ref.calls == new and s_ref.steps == 0 and torch.equal(out_ref[:, :T0 + 2], out0)
    assert int(out_ref[:, T0:].max()) < cfg["image_start_id"]
    # switched on: one prefill, new - 1 decode steps, teacher-forced on the loop's tokens
    assert model.enable_kv_cache() is model and eng.supports_kv_cache and not type(eng).supports_kv_cache
    out, s = cached_run(model, kw, monkeypatch, replay(out_ref, T0), max_new_tokens=new)
    assert s.calls == 1 and s.steps == new - 1, "one forward_hidden, new - 1 decode steps"
    assert s.names.count("vlr_decoder_layer_decode") == (new - 1) * eng.L
    assert torch.equal(out, out_ref) and len(s.logits) == len(s_ref.logits) == new
    assert torch.equal(s.logits[0][:B], s_ref.logits[0][:B]), "first step: same prefill, same lm-head call"
    for k in range(1, new):
        e = relerr(s.logits[k][:B], s_ref.logits[k][:B])
        print(f"qwenvl step {k}: cached vs re-forward loop rel err {e:.3e} (bound 2e-2)")
        assert e < 2e-2, (k, e)
    # free-running: the tokens agree (the first two firmly, as on LLaVA; later ones unless a bf16 near-tie moved the prefix)
    free, _ = cached_run(model, kw, monkeypatch, below_markers(cfg), max_new_tokens=new)
    assert torch.equal(free[:, :T0 + 2], out_ref[:, :T0 + 2])
    # switched off again: the loop
    model.enable_kv_cache(False)
    _, s_off = cached_run(model, kw, monkeypatch, below_markers(cfg), max_new_tokens=2)
    assert s_off.calls == 2 and s_off.steps == 0


def test_stop_words_end_rows_as_on_the_loop(gpu, monkeypatch):
    """Qwen-VL-Chat's stop words (prepare_default_generation_kwargs) plus one the fixture can emit: row 0's third token"""
    cfg, model, kw = qwen(gpu)
    T0 = kw["input_ids"].shape[1]
    free, _ = loop_run(model, kw, cfg, monkeypatch, max_new_tokens=5)
    gk = model.prepare_default_generation_kwargs(SimpleNamespace(max_new_tokens=5, eos_token_id=NO_EOS, pad_token_id=PAD))
    gc = gk["generation_config"]
    assert gc.stop_words_ids == [[151645], [151644]]
    gc.stop_words_ids = gc.stop_words_ids + [[int(free[0, T0 + 2])]]
    gc.do_sample = True
    kw = {k: v for k, v in kw.items() if k not in ("do_sample", "pad_token_id", "eos_token_id")}
    out_ref, s_ref = loop_run(model, kw, cfg, monkeypatch, **gk)
    model.enable_kv_cache()
    out, s = cached_run(model, kw, monkeypatch, replay(out_ref, T0), **gk)
    assert s.calls == 1 and s.steps >= 1
    assert torch.equal(out, out_ref)
    hit = int((out[0, T0:] == int(free[0, T0 + 2])).nonzero()[0])
    assert hit <= 2 and bool((out[0, T0 + hit + 1:] == PAD).all()), "the stop token stays, the row receives the pad id afterwards"


def test_live_merged_and_disabled_adapters(gpu, monkeypatch):
    cfg, model, kw = qwen(gpu, lora=True)
    eng, new = model.engine, 3
    B, T0 = kw["input_ids"].shape
    out_ref, s_ref = loop_run(model, kw, cfg, monkeypatch, max_new_tokens=new)
    model.enable_kv_cache()
    # live: nothing merged, first logits bit for bit, later steps within the bound
    monkeypatch.setattr(eng, "merged_weights", lambda *a, **k: pytest.fail("merge_lora=False cloned and merged the policy"))
    out, s = cached_run(model, kw, monkeypatch, replay(out_ref, T0), max_new_tokens=new, merge_lora=False)
    assert s.calls == 1 and s.ws[0] is eng.policy and s.steps == new - 1
    assert s.names.count("vlr_decoder_layer_decode_lora") == (new - 1) * eng.L and "vlr_decoder_layer_decode" not in s.names
    assert torch.equal(s.logits[0][:B], s_ref.logits[0][:B]), "live adapters: the prefill is the loop's first forward"
    for k in range(1, new):
        e = relerr(s.logits[k][:B], s_ref.logits[k][:B])
        print(f"qwenvl live adapters step {k}: rel err {e:.3e} (bound 2e-2)")
        assert e < 2e-2, (k, e)
    # merged: a second weight set, within bf16 rounding of the un-merged loop (rule of test_cached_generate_with_lora_policy...)
    out, s = cached_run(model, kw, monkeypatch, replay(out_ref, T0), max_new_tokens=new)
    assert s.calls == 1 and s.ws[0] is not eng.policy and s.steps == new - 1 and "vlr_decoder_layer_decode_lora" not in s.names
    for k in range(new):
        e = relerr(s.logits[k][:B], s_ref.logits[k][:B])
        print(f"qwenvl merged adapters step {k}: rel err {e:.3e} (bound 2e-2)")
        assert e < 2e-2, (k, e)
    # disabled: the base weights, adapter-free calls, first logits bit for bit
    with model.disable_adapter():
        model.enable_kv_cache(False)
        off_ref, so_ref = loop_run(model, kw, cfg, monkeypatch, max_new_tokens=new)
        model.enable_kv_cache()
        off, so = cached_run(model, kw, monkeypatch, replay(off_ref, T0), max_new_tokens=new, merge_lora=False)
    assert so.calls == 1 and so.ws[0] is eng.policy and not [n for n in so.names if n.endswith("_lora")]
    assert torch.equal(so.logits[0][:B], so_ref.logits[0][:B])
    assert not torch.equal(so.logits[0][:B], s_ref.logits[0][:B]), "the adapters change the logits"
    for k in range(1, new):
        assert relerr(so.logits[k][:B], so_ref.logits[k][:B]) < 2e-2


def test_num_return_sequences_over_the_shared_prompt_cache(gpu, monkeypatch):
    """three samples per prompt over a SharedPromptKVCache against the cached route on the expanded batch, teacher-forced (bound and
    helper of tests/test_hip_decode_shared.py); a sampled image-marker id is a plain token on both"""
    cfg, model, kw = qwen(gpu)
    model.enable_kv_cache()
    names = []
    from vlrlhf import _hip
    call = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    out = model.generate(num_return_sequences=3, max_new_tokens=3, generator=torch.Generator(device=gpu).manual_seed(11), **kw)
    monkeypatch.undo()
    assert out.shape == (6, kw["input_ids"].shape[1] + 3) and names.count("vlr_decoder_layer_decode_shared") == 2 * model.engine.L
    teacher_forced_parity(model, kw, gpu, monkeypatch)


def test_twenty_rows_take_the_wide_gemms_and_give_the_bits_of_the_groups(gpu, monkeypatch):
    """a 20-row batch: the decode scratch is sized for 64-row groups, every skinny GEMM of a step is one wide call; withholding the wide
    scratch (engine.wide_gemv = False: 16-row groups, the parent's calls) gives the same logits and tokens bit for bit"""
    cfg, model, kw = qwen(gpu, repeat=10)
    model.enable_kv_cache()
    eng, new = model.engine, 4
    assert kw["input_ids"].shape[0] == 20 and eng.wide_gemv
    wide, sw = cached_run(model, kw, monkeypatch, below_markers(cfg), max_new_tokens=new)
    assert sw.calls == 1 and sw.steps == new - 1
    assert sw.names.count("vlr_gemv_wide_bf16") == new - 1 and "vlr_gemv_bf16" not in sw.names, "the lm-head: one wide call per step"
    eng.wide_gemv = False
    groups, sg = cached_run(model, kw, monkeypatch, below_markers(cfg), max_new_tokens=new)
    assert sg.names.count("vlr_gemv_bf16") == 2 * (new - 1) and "vlr_gemv_wide_bf16" not in sg.names
    assert torch.equal(wide, groups) and len(sw.logits) == len(sg.logits) == new
    for a, b in zip(sw.logits, sg.logits):
        assert torch.equal(a, b)
    assert torch.equal(wide[:2], wide[2:4]), "repeated rows decode alike"


def test_decode_step_embeds_an_image_marker_id_as_a_plain_token(gpu):
    """modeling_qwen.py:525 looks for images only without past_key_values: a NEW token whose id is <img>, </img> or the pad slot is a
    wte row to decode_step (the re-forward loop raises on an unbalanced marker)"""
    cfg, model, kw = qwen(gpu)
    model.enable_kv_cache()
    eng = model.engine
    ids, mask = kw["input_ids"], kw["attention_mask"]
    fill = torch.full((2, 2), PAD, dtype=ids.dtype, device=gpu)
    run_ids, run_mask = torch.cat([fill, ids], 1), torch.cat([torch.zeros_like(fill), mask], 1)      # 32 columns
    cache = eng.new_kv_cache(2, 3)
    with torch.no_grad():
        eng.forward_hidden(model.weights, run_ids, run_mask, None, kw["pixel_values"], kv_cache=cache)
        assert cache.len == 32 and cache.pos.tolist() == [32, 32], "left-padded rows decode at the column index"
        st = cfg["image_start_id"]
        for step, tok in enumerate(([st, st + 1], [st + 2, st], [st + 1, 300])):
            logits = eng.decode_step(model.weights, torch.tensor(tok, device=gpu), cache)
            assert logits.shape == (2, cfg["vocab"]) and torch.isfinite(logits).all()
            assert cache.len == 33 + step and cache.pos.tolist() == [33 + step] * 2
    with pytest.raises(ValueError):                           # the loop, on the same ids: an unbalanced <img>
        bad = torch.cat([ids, torch.full((2, 1), st, dtype=ids.dtype, device=gpu)], 1)
        model(input_ids=bad, attention_mask=torch.ones_like(bad), pixel_values=kw["pixel_values"])


def test_packed_int4_base_decodes_through_the_w4_calls(gpu, tmp_path, monkeypatch):
    """a GPTQ checkpoint (Qwen-VL-Chat-Int4's layout) stays packed: the prefill dequantises layer by layer and equals the bf16 model on
    the dequantised weights bit for bit; the decode steps run vlr_decoder_layer_decode_w4 and stay within 1e-4 relative of that model's
    (same bf16 products, fp32 sums in another order: the bound of test_decode_from_packed_weights)"""
    from tests import gptq_ref as R
    from vlrlhf.models.QwenVL import QwenVLForRL, _hf_from_cfg
    cfg, _, kw = qwen(gpu)
    W = load_case("qwenvl_small")[2]
    deq = R.write_checkpoint(str(tmp_path), _hf_from_cfg(dict(cfg, family="qwen_vl")), W, 32)
    A = QwenVLForRL.from_pretrained(str(tmp_path))
    B = QwenVLForRL.from_state_dict({k: v for k, v in A.engine.cfg.items() if k != "gptq"}, deq)
    assert A.is_packed and not B.is_packed
    new, (rows, T0) = 4, kw["input_ids"].shape
    for m in (A, B):
        m.eval()
        m.enable_kv_cache()
    out_b, sb = cached_run(B, kw, monkeypatch, below_markers(cfg), max_new_tokens=new)
    out_a, sa = cached_run(A, kw, monkeypatch, replay(out_b, T0), max_new_tokens=new)
    assert sa.calls == 1 and sa.steps == new - 1 and sa.names.count("vlr_decoder_layer_decode_w4") == (new - 1) * A.engine.L
    assert "vlr_decoder_layer_decode" not in sa.names and torch.equal(out_a, out_b)
    assert torch.equal(sa.logits[0][:rows], sb.logits[0][:rows]), "the prefill dequantises: the bf16 model's bits"
    for k in range(1, new):
        e = relerr(sa.logits[k][:rows], sb.logits[k][:rows])
        print(f"qwenvl packed step {k}: packed vs dequantised bf16 rel err {e:.3e} (bound 1e-4)")
        assert e < 1e-4, (k, e)
