"""InternLM-XComposer2 on the KV cache, switched on by the caller (InternLMXC2ForRL.enable_kv_cache), end to end on the MI355X with the
internlmxc2_small fixture (heads 2, kv_heads 1, head_dim 128).  The yardsticks are the model's own re-forward loop (use_cache=False:
what a fresh model does) fed the SAME tokens, and the fp32 oracle (oracle/internlm_oracle.py).  The loop rejects a generated
<ImageHere> id on its next re-forward (one more image token than images), so tokens are chosen by a stand-in for torch.multinomial that
takes the most likely id BELOW the image token (both routes run with do_sample=True and see the same stand-in); the cached route is
then teacher-forced on the loop's tokens.  Bounds are the project's: first-step logits bit for bit, later steps 2e-2 relative
(tests/test_hip_decode.py::test_cached_generate_matches_reforward_loop), greedy tokens within 0.06 of the oracle's logit range
(test_cached_greedy_tokens_against_oracle).  Needs a real MI355X:  pytest -m gpu"""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import internlm_oracle as IL  # noqa: E402  (checker only)
from tests.golden_util import load_case  # noqa: E402
from tests.test_hip_decode_lora import PEFT, Spy, relerr, wake_adapters  # noqa: E402
from tests.test_hip_decode_qwenvl import cached_run, replay  # noqa: E402
from tests.test_hip_decode_shared import teacher_forced_parity  # noqa: E402
from tests.test_hip_decode_wide_kernels import DEV, layer_case, same_bits, scratch  # noqa: E402

PAD, NO_EOS, NEW = 2, 10 ** 6, 7


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return torch.device("cuda")


def prompts():
    """-> (cfg, W, ids, mask, pixels) on the host: the fixture's two prompts (11 and 14 tokens, each with its <ImageHere>), LEFT-padded"""
    z, cfg, W, W_ref, batch, _ = load_case("internlmxc2_small")
    src, lens, T = batch["chosen_input_ids"], (11, 14), 14
    ids = torch.full((2, T), PAD, dtype=torch.long)
    mask = torch.zeros(2, T, dtype=torch.long)
    for i, n in enumerate(lens):
        assert bool((batch["chosen_labels"][i, :n] == -100).all()), "prompt tokens only"
        ids[i, T - n:] = src[i, :n]
        mask[i, T - n:] = 1
    assert int((ids == cfg["image_token"]).sum()) == 2 and bool((mask[:, 0] == 0).any()) and int(mask[0].sum()) != int(mask[1].sum())
    return cfg, W, ids, mask, batch["img_input_dict"]["pixel_values"]


def ilm(gpu, lora=False):
    from vlrlhf.models.InternLMXC2 import InternLMXC2ForRL
    cfg, W, ids, mask, px = prompts()
    model = InternLMXC2ForRL.from_state_dict(cfg, W)
    if lora:
        model.apply_lora(dict(PEFT, r=8))
        wake_adapters(model)
    model.eval()
    kw = dict(input_ids=ids.to(gpu), attention_mask=mask.to(gpu), pixel_values=px.to(gpu), do_sample=True, pad_token_id=PAD, eos_token_id=NO_EOS)
    return cfg, model, kw


def below_image_token(cfg):
    """stand-in for torch.multinomial: the most likely id below the image token (ids the re-forward loop can embed again)"""
    return lambda probs, num, generator=None: probs[:, :cfg["image_token"]].argmax(-1, keepdim=True)


def loop_run(model, kw, cfg, monkeypatch, **extra):
    """the re-forward loop on restricted-greedy tokens -> (ids, spy)"""
    s = Spy(model, monkeypatch)
    monkeypatch.setattr(torch, "multinomial", below_image_token(cfg))
    out = model.generate(use_cache=False, **kw, **extra)
    monkeypatch.undo()
    return out, s


def within_the_loop(s, s_ref, B, what, first_equal=True):
    assert len(s.logits) == len(s_ref.logits)
    if first_equal:
        assert torch.equal(s.logits[0][:B], s_ref.logits[0][:B]), f"{what}: first step - same prefill, same lm-head call"
    for k in range(0 if not first_equal else 1, len(s.logits)):
        e = relerr(s.logits[k][:B], s_ref.logits[k][:B])
        print(f"internlm {what} step {k}: cached vs re-forward loop rel err {e:.3e} (bound 2e-2)")
        assert e < 2e-2, (what, k, e)


def test_generation_matches_the_reforward_loop(gpu, monkeypatch):
    """a fresh model re-forwards and makes no decode_step; switched on: ONE prefill, then 6 decode steps, first logits bit for bit, later
    ones within 2e-2 of the loop's on the same prefix; two left-padded prompts of unequal length"""
    cfg, model, kw = ilm(gpu)
    eng = model.engine
    B, T0 = kw["input_ids"].shape
    assert not eng.supports_kv_cache and eng.nh == 2 and eng.nkv == 1 and eng.hd == 128
    out0, s0 = cached_run(model, kw, monkeypatch, below_image_token(cfg), max_new_tokens=2)
    assert s0.calls == 2 and s0.steps == 0, "a fresh model runs the re-forward loop"
    out_ref, s_ref = loop_run(model, kw, cfg, monkeypatch, max_new_tokens=NEW)
    assert s_ref.calls == NEW and s_ref.steps == 0 and torch.equal(out_ref[:, :T0 + 2], out0)
    assert int(out_ref[:, T0:].max()) < cfg["image_token"]
    assert model.enable_kv_cache() is model and eng.supports_kv_cache and not type(eng).supports_kv_cache
    out, s = cached_run(model, kw, monkeypatch, replay(out_ref, T0), max_new_tokens=NEW)
    assert s.calls == 1 and s.steps == NEW - 1 == 6, "one forward_hidden, six decode steps"
    assert s.names.count("vlr_decoder_layer_decode") == (NEW - 1) * eng.L and s.names.count("vlr_decoder_layer_fwd_lora_ex") == eng.L, \
        "the prefill runs the engine's own layer call: PLoRA on the image rows"
    assert torch.equal(out, out_ref) and len(s.logits) == NEW
    within_the_loop(s, s_ref, B, "full fine-tune weights")
    # free-running: the tokens agree (the first two firmly, as on LLaVA; later ones unless a bf16 near-tie moved the prefix)
    free, _ = cached_run(model, kw, monkeypatch, below_image_token(cfg), max_new_tokens=NEW)
    assert torch.equal(free[:, :T0 + 2], out_ref[:, :T0 + 2])
    model.enable_kv_cache(False)
    _, s_off = cached_run(model, kw, monkeypatch, below_image_token(cfg), max_new_tokens=2)
    assert s_off.calls == 2 and s_off.steps == 0, "switched off again: the loop"


def test_left_padded_rows_decode_where_the_loop_puts_them(gpu):
    """the prefill of 32 token columns merges to S columns; both rows - 3 pad columns apart - append at position S, S + 1, ..."""
    cfg, model, kw = ilm(gpu)
    model.enable_kv_cache()
    eng = model.engine
    ids, mask = kw["input_ids"], kw["attention_mask"]
    fill = torch.full((2, 32 - ids.shape[1]), PAD, dtype=ids.dtype, device=gpu)
    run_ids, run_mask = torch.cat([fill, ids], 1), torch.cat([torch.zeros_like(fill), mask], 1)
    S = 32 + (cfg["image_size"] // cfg["patch_size"]) ** 2 - 1
    cache = eng.new_kv_cache(2, 2)
    with torch.no_grad():
        c = eng.forward_hidden(model.weights, run_ids, run_mask, None, kw["pixel_values"], kv_cache=cache)
        assert c["S"] == S and cache.len == S and cache.pos.tolist() == [S, S]
        assert int(cache.key_mask[0, :S].sum()) + 3 == int(cache.key_mask[1, :S].sum())
        for step in range(2):
            logits = eng.decode_step(model.weights, torch.tensor([5, 7], device=gpu), cache)
            assert logits.shape == (2, cfg["vocab"]) and torch.isfinite(logits).all()
            assert cache.len == S + 1 + step and cache.pos.tolist() == [S + 1 + step] * 2


def test_greedy_tokens_against_the_fp32_oracle(gpu, monkeypatch):
    """the cached route's tokens judged against the fp32 oracle's teacher-forced next-token logits, PLoRA on the image rows included:
    the chosen token is within 0.06 of the oracle's logit range of the oracle's best id (among the ids the stand-in may choose)"""
    cfg, model, kw = ilm(gpu)
    model.enable_kv_cache()
    _, W, ids0, m0, px = prompts()
    T0, new = ids0.shape[1], 6
    out, s = cached_run(model, kw, monkeypatch, below_image_token(cfg), max_new_tokens=new)
    out = out.cpu()
    assert s.calls == 1 and s.steps == new - 1 and out.shape == (2, T0 + new) and torch.equal(out[:, :T0], ids0)
    ids, mask = ids0.clone(), m0.clone()
    for k in range(new):
        logits, _, aux = IL.internlm_forward(W, cfg, ids, mask, torch.full_like(ids, -100), px, dedupe_images=False)
        for b in range(2):
            last = int(torch.nonzero(aux["mask"][b]).max())
            row = logits[b, last]
            tok = int(out[b, T0 + k])
            best = row[:cfg["image_token"]].max()
            gap, rng = float(best - row[tok]), float(row.max() - row.min())
            print(f"internlm oracle step {k} row {b}: token {tok}, oracle best {int(row[:cfg['image_token']].argmax())}, gap {gap:.4f} of range {rng:.4f}")
            assert gap <= 0.06 * rng, (k, b, tok, int(row.argmax()))
        ids = torch.cat([ids, out[:, T0 + k: T0 + k + 1]], 1)
        mask = torch.cat([mask, torch.ones(2, 1, dtype=mask.dtype)], 1)


def test_live_merged_and_disabled_adapters(gpu, monkeypatch):
    """peft LoRA over the frozen PLoRA decoder, each route against the loop under the same route"""
    cfg, model, kw = ilm(gpu, lora=True)
    eng, new = model.engine, 4
    assert eng.lora_fused and eng.lora_layout.qkv_targets == 1
    B, T0 = kw["input_ids"].shape
    out_ref, s_ref = loop_run(model, kw, cfg, monkeypatch, max_new_tokens=new)
    assert s_ref.names.count("vlr_decoder_layer_fwd_lora2") == new * eng.L
    model.enable_kv_cache()
    # live: nothing merged; the prefill is the loop's first forward (two adapters per projection), the steps run the peft adapters alone
    monkeypatch.setattr(eng, "merged_weights", lambda *a, **k: pytest.fail("merge_lora=False cloned and merged the policy"))
    out, s = cached_run(model, kw, monkeypatch, replay(out_ref, T0), max_new_tokens=new, merge_lora=False)
    assert s.calls == 1 and s.ws[0] is eng.policy and s.steps == new - 1
    assert s.names.count("vlr_decoder_layer_decode_lora") == (new - 1) * eng.L and "vlr_decoder_layer_decode" not in s.names
    assert s.names.count("vlr_decoder_layer_fwd_lora2") == eng.L
    within_the_loop(s, s_ref, B, "live adapters")
    # merged: a second weight set (PLoRA stays un-merged and active in its prefill), within bf16 rounding of the un-merged loop
    out, s = cached_run(model, kw, monkeypatch, replay(out_ref, T0), max_new_tokens=new)
    assert s.calls == 1 and s.ws[0] is not eng.policy and s.steps == new - 1 and "vlr_decoder_layer_decode_lora" not in s.names
    assert s.names.count("vlr_decoder_layer_fwd_lora_ex") == eng.L
    within_the_loop(s, s_ref, B, "merged adapters", first_equal=False)
    # disabled: the base weights with PLoRA active in the prefill, adapter-free steps, first logits bit for bit
    with model.disable_adapter():
        model.enable_kv_cache(False)
        off_ref, so_ref = loop_run(model, kw, cfg, monkeypatch, max_new_tokens=new)
        model.enable_kv_cache()
        off, so = cached_run(model, kw, monkeypatch, replay(off_ref, T0), max_new_tokens=new, merge_lora=False)
    assert so.calls == 1 and so.ws[0] is eng.policy and not [n for n in so.names if n.endswith("_lora")]
    assert so.names.count("vlr_decoder_layer_fwd_lora_ex") == eng.L
    assert not torch.equal(so.logits[0][:B], s_ref.logits[0][:B]), "the adapters change the logits"
    within_the_loop(so, so_ref, B, "disabled adapters")


def test_composed_layers_keep_the_loop(gpu, monkeypatch):
    """VLR_ILM_LORA_FUSED=0, adapters applied AFTER the switch: generate re-forwards, the switch stands"""
    monkeypatch.setenv("VLR_ILM_LORA_FUSED", "0")
    cfg, model, kw = ilm(gpu)
    model.enable_kv_cache()
    model.apply_lora(dict(PEFT, r=8))
    model.eval()
    eng = model.engine
    assert not eng.lora_fused and not eng.kv_cache_layers and eng.supports_kv_cache
    out, s = cached_run(model, kw, monkeypatch, below_image_token(cfg), max_new_tokens=2)
    assert s.calls == 2 and s.steps == 0 and eng.supports_kv_cache and out.shape[1] == kw["input_ids"].shape[1] + 2


def test_num_return_sequences_over_the_shared_prompt_cache(gpu, monkeypatch):
    """three samples per prompt over a SharedPromptKVCache against the cached route on the expanded batch, teacher-forced (bound and
    helper of tests/test_hip_decode_shared.py); a sampled <ImageHere> id is a plain token to both"""
    cfg, model, kw = ilm(gpu)
    model.enable_kv_cache()
    names = []
    from vlrlhf import _hip
    call = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    out = model.generate(num_return_sequences=3, max_new_tokens=3, generator=torch.Generator(device=gpu).manual_seed(11), **kw)
    monkeypatch.undo()
    assert out.shape == (6, kw["input_ids"].shape[1] + 3) and names.count("vlr_decoder_layer_decode_shared") == 2 * model.engine.L
    teacher_forced_parity(model, kw, gpu, monkeypatch)


def test_run_vqa_reaches_decode_step(gpu, tmp_path, monkeypatch):
    """eval.utils.load_model_and_processor on a saved checkpoint switches the cache on (the method exists), so run_vqa's answers come
    from one prefill and decode steps - the tokens of a direct cached generate"""
    import vlrlhf.eval.utils as U
    import vlrlhf.utils.auto_load as AL
    from vlrlhf.engine_internlm import InternLMHipEngine
    from vlrlhf.models.InternLMXC2 import InternLMXC2ForRL
    cfg, model, kw = ilm(gpu)
    model.save_pretrained(str(tmp_path))
    gen = dict(max_new_tokens=4, do_sample=False, pad_token_id=PAD, eos_token_id=NO_EOS)
    model.enable_kv_cache()
    direct = model.generate(**{k: v for k, v in kw.items() if k in ("input_ids", "attention_mask", "pixel_values")}, **gen)
    T0 = kw["input_ids"].shape[1]
    tok = SimpleNamespace(batch_decode=lambda rows, **k: [" ".join(str(int(i)) for i in row) for row in rows])
    monkeypatch.setattr(AL.MyAutoProcessor, "from_pretrained", classmethod(lambda cls, path, **k: SimpleNamespace(tokenizer=tok, infer=lambda: None)))
    monkeypatch.setattr(InternLMXC2ForRL, "prepare_default_generation_kwargs", lambda self, gc: dict(gen))
    steps, prefills = [], []
    ds, fh = InternLMHipEngine.decode_step, InternLMHipEngine.forward_hidden
    monkeypatch.setattr(InternLMHipEngine, "decode_step", lambda self, *a, **k: (steps.append(1), ds(self, *a, **k))[1])
    monkeypatch.setattr(InternLMHipEngine, "forward_hidden", lambda self, *a, **k: (prefills.append(1), fh(self, *a, **k))[1])

    class Rows(U.VLCollator):
        def __call__(self, rows):
            idx = torch.tensor([r["row"] for r in rows], device=gpu)
            return dict(input_ids=kw["input_ids"][idx], attention_mask=kw["attention_mask"][idx], pixel_values=kw["pixel_values"][idx]), \
                [dict(row=r["row"]) for r in rows]

    U.get_model_cache().clear()
    try:
        out = U.run_vqa(str(tmp_path), [dict(row=0), dict(row=1)], Rows, None, None, 16)
        loaded = U.get_model_cache()[(str(tmp_path), "None")][0]
        assert isinstance(loaded, InternLMXC2ForRL) and loaded is not model and loaded.engine.supports_kv_cache
    finally:
        U.get_model_cache().clear()
    assert len(prefills) == 1 and len(steps) == 3, "one prefill, then a decode step per further token"
    assert [o["response"] for o in out] == [" ".join(str(int(i)) for i in row) for row in direct[:, T0:]]
    assert [o["row"] for o in out] == [0, 1]


# ---- the adapter layout this family sends through the decode kernels: ONE adapter over the fused wqkv (qkv_targets = 1) AND a `down`
# adapter, at grouped-query widths.  No other family has it (Qwen-VL: 1 without down; LLaVA: 3 with down), so it is pinned at kernel
# level: with the single A block repeated three times the 3-target call - the combination tests/test_hip_decode_lora_kernels.py and
# tests/test_hip_decode_wide_kernels.py hold against fp64 and against the 16-row groups - reads the same u columns and must give the
# same bits (x A^T takes one K slice at hidden 256 whether A has r or 3 r rows).
def run_layer(hip, c, qkv_targets, a_qkv, b_qkv, wide, resid_f32=1):
    H, I, nh, nkv, B, N, Nq, r = (c[k] for k in ("H", "I", "nh", "nkv", "B", "N", "Nq", "r"))
    lib = hip.lib()
    cfg = hip.LlamaCfg(H, I, nh, c["hd"], 1e-5, c["max_pos"], c["cos"].data_ptr(), c["sin"].data_ptr(), nkv, resid_f32)
    lw = hip.LayerWeights(*(c["W"][k].data_ptr() for k in ("ln1", "wqkv", "wo", "ln2", "wgu", "wdown", "bqkv")))
    shapes, rt = ((N, H), (H, Nq), (2 * I, H), (H, I)), (qkv_targets * r, r, 2 * r, r)
    fw, fu = (lib.vlr_gemv_wide_lora_workspace_bytes, lib.vlr_gemv_wide_lora_u_bytes) if wide else \
        (lib.vlr_gemv_lora_workspace_bytes, lib.vlr_gemv_lora_u_bytes)
    mb = min(B, 64) if wide else 16
    gb = max(int(fw(mb, n, k, t)) for (n, k), t in zip(shapes, rt))
    ub = max(int(fu(mb, k, t)) for (n, k), t in zip(shapes, rt))
    ab = int(lib.vlr_attn_decode_workspace_bytes(B, nh, c["cap"]))
    d = dict(xn=torch.empty(B, H, dtype=torch.bfloat16, device=DEV), rstd=torch.empty(B, device=DEV),
             qkv=torch.empty(B, N, dtype=torch.bfloat16, device=DEV), attn=torch.empty(B, Nq, dtype=torch.bfloat16, device=DEV),
             act=torch.empty(B, I, dtype=torch.bfloat16, device=DEV), gemv=scratch(gb), attn_ws=torch.empty(ab, dtype=torch.uint8, device=DEV))
    dws = hip.DecodeWs(d["xn"].data_ptr(), d["rstd"].data_ptr(), d["qkv"].data_ptr(), d["attn"].data_ptr(), d["act"].data_ptr(),
                       d["gemv"].data_ptr(), gb, d["attn_ws"].data_ptr(), ab)
    x = c["x"].to(torch.float32 if resid_f32 else torch.bfloat16).clone()
    kc, vc = c["kc"].clone(), c["vc"].clone()
    u = scratch(ub)
    lws = hip.DecodeLoraWs(u.data_ptr(), ub)
    Ad = dict(c["Ad"], a_qkv=a_qkv, b_qkv=b_qkv)
    lo = hip.LoraWeights(r, 2.0, 0.0, *(Ad[k].data_ptr() for k in ("a_qkv", "b_qkv", "a_o", "b_o", "a_gu", "b_gu", "a_down", "b_down")),
                         qkv_targets, None)
    hip.call("vlr_decoder_layer_decode_lora", cfg, lw, lo, dws, lws, x, c["pos"], kc, vc, c["km"], B, c["cap"], c["S"])
    torch.cuda.synchronize()
    return x, kc[:, :, c["S"]].clone(), vc[:, :, c["S"]].clone()


@pytest.mark.parametrize("resid_f32", [1, 0])
def test_one_adapter_over_fused_qkv_with_a_down_adapter_at_kernel_level(gpu, resid_f32):
    from vlrlhf import _hip as hip
    c = layer_case(hip, 256, 256, 2, 1)                       # 33 rows, heads 2, kv_heads 1, head_dim 128: the fixture's widths
    r = c["r"]
    a1 = c["Ad"]["a_qkv"][:r].contiguous()
    a3 = a1.repeat(3, 1).contiguous()
    b = c["Ad"]["b_qkv"]
    runs = {(t, wide): run_layer(hip, c, t, a, b, wide, resid_f32) for t, a in ((1, a1), (3, a3)) for wide in (False, True)}
    base = runs[(3, False)]
    assert all(torch.isfinite(t.float()).all() for t in base)
    for key, got in runs.items():
        for what, g, w in zip(("x_inout", "the new K column", "the new V column"), got, base):
            same_bits(g, w, f"qkv_targets {key[0]}, {'64-row groups' if key[1] else '16-row groups'}: {what}")
    off = run_layer(hip, c, 1, a1, torch.zeros_like(b), False, resid_f32)
    assert not torch.equal(off[1], base[1]) and not torch.equal(off[0], base[0]), "the adapter over the fused rows reaches k and the stream"
