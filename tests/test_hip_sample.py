"""generate(sampler="device") end to end on the MI355X, on the small LLaVA-1.5 and Qwen-VL fixtures of the decode tests: greedy equals
top_k = 1 equals the torch sampler's greedy; the draw is a function of (seed, call); sync_every does not change the output; every token
and log-prob is replayed on the host (tests/sample_ref.py) from the logits captured at each step; the fan-out reads the prompt through
prompt_div; a generation config's warper settings reach the kernel; a default generate never launches it; and a GRPO run with
device_sampler, interrupted and resumed, lands on the uninterrupted run's bits.  Needs a real MI355X:  pytest -m gpu"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import sample_ref as SR  # noqa: E402
from tests.test_hip_decode import Spy, gpu, llava, prompt_kw  # noqa: E402,F401
from tests.test_hip_decode_qwenvl import qwen  # noqa: E402

NO_EOS = 10 ** 6


@pytest.fixture(scope="module")
def small(gpu):
    cfg, W, batch, model = llava("llava_hipsmall")
    model.eval()
    return cfg, model, dict(prompt_kw(batch, gpu), pad_token_id=0, eos_token_id=NO_EOS)


def dev_gen(model, kw, call=0, **extra):
    """generate(sampler="device") under a chosen call word"""
    model._sampler_calls = call
    return model.generate(sampler="device", **kw, **extra)


def test_top_k_1_is_greedy_on_both_samplers(small):
    cfg, model, kw = small
    for cache in (True, False):
        want = model.generate(do_sample=False, max_new_tokens=5, use_cache=cache, **kw)
        a = dev_gen(model, kw, do_sample=True, top_k=1, temperature=0.7, seed=5, max_new_tokens=5, use_cache=cache)
        b = dev_gen(model, kw, do_sample=False, max_new_tokens=5, use_cache=cache)
        assert torch.equal(a, want) and torch.equal(b, want), cache
        assert a.dtype == want.dtype and a.is_contiguous()


def test_top_k_1_is_greedy_on_qwenvl_cache(gpu):
    cfg, model, kw = qwen(gpu)
    model.enable_kv_cache()
    kw = dict(kw, do_sample=False)
    want = model.generate(max_new_tokens=5, **kw)
    assert torch.equal(dev_gen(model, kw, max_new_tokens=5), want)
    assert torch.equal(dev_gen(model, dict(kw, do_sample=True), top_k=1, seed=3, max_new_tokens=5), want)


def test_draw_is_a_function_of_seed_and_call(small):
    cfg, model, kw = small
    g = dict(do_sample=True, top_k=0, temperature=1.5, max_new_tokens=8)
    a = dev_gen(model, kw, call=4, seed=11, **g)
    assert model._sampler_calls == 5                            # one bump per call
    assert torch.equal(dev_gen(model, kw, call=4, seed=11, **g), a)
    assert not torch.equal(dev_gen(model, kw, call=4, seed=12, **g), a)
    assert not torch.equal(dev_gen(model, kw, call=5, seed=11, **g), a)
    gen = torch.Generator(device="cuda").manual_seed(11)
    assert torch.equal(dev_gen(model, kw, call=4, generator=gen, **g), a)      # seed = the generator's initial seed


def test_sync_every_does_not_change_the_output(small):
    """rows that stop at different columns - one by an eos id, one by a stop sequence - and the host looking every 1 / 3 / 8 tokens"""
    cfg, model, kw = small
    g = dict(do_sample=True, top_k=0, temperature=1.5, seed=21, max_new_tokens=12)
    free = dev_gen(model, kw, **g)
    B, T = kw["input_ids"].shape
    assert free.shape == (B, T + 12)
    eos = int(free[0, T + 2])                                   # row 0 ends at its third token (or earlier, should it repeat)
    stop = [int(free[1, T + 3]), int(free[1, T + 4])]           # row 1 at its fifth, by a two-token stop sequence
    gc = SimpleNamespace(stop_words_ids=[stop], max_new_tokens=12)
    kw2 = dict(kw, eos_token_id=eos)
    outs = [dev_gen(model, kw2, generation_config=gc, sync_every=s, output_logprobs=True, **{k: v for k, v in g.items() if k != "max_new_tokens"})
            for s in (1, 3, 8)]
    ids, lp = outs[0]
    for o_ids, o_lp in outs[1:]:
        assert torch.equal(o_ids, ids) and torch.equal(o_lp, lp)
    gen = ids[:, T:].cpu()
    ends = []
    for r in range(B):
        row, end = gen[r].tolist(), None
        for t in range(len(row)):
            if row[t] == eos or (t >= 1 and row[t - 1:t + 1] == stop):
                end = t
                break
        ends.append(end)
        if end is not None:
            assert all(x == 0 for x in row[end + 1:]) and bool((lp[r, end + 1:] == 0).all()), "pad id and log-prob 0 after the stop"
    assert ends[0] is not None and ends[0] <= 2 and ends[1] is not None and ends[1] <= 4
    if all(e is not None for e in ends):                        # everyone stopped: trimmed where a per-token check would have stopped
        assert gen.shape[1] == max(ends) + 1
    else:
        assert gen.shape[1] == 12
    assert torch.equal(ids[:, T], free[:, T])                   # the same draws: a stop changes nothing before it


def replay_on_host(model, kw, monkeypatch, fanout=1, new=6, **g):
    """generate on the device sampler with the per-step logits captured (Spy) -> every token, log-prob and flag against sample_ref"""
    model._sampler_calls = 9
    s = Spy(model, monkeypatch)
    ids, lp = model.generate(sampler="device", output_logprobs=True, max_new_tokens=new, **kw, **g,
                             **({"num_return_sequences": fanout} if fanout > 1 else {}))
    monkeypatch.undo()
    P, T = kw["input_ids"].shape
    rows = P * fanout
    new = ids.shape[1] - T                                      # (trimmed when every row stopped early)
    assert 1 <= new and lp.shape == (rows, new) and len(s.logits) >= new
    gen, lp = ids[:, T:].cpu().numpy(), lp.cpu().numpy()
    unf, fin = np.ones(rows, dtype=np.uint8), np.full(rows, -1, dtype=np.int32)
    worst = 0.0
    for n in range(new):
        x = s.logits[n].float().cpu()
        x = (x[:P].repeat_interleave(fanout, 0) if n == 0 else x[:rows]).numpy()      # the prefill's logits are repeated, as generate does
        ref = SR.sample_ref(x, do_sample=g.get("do_sample", False), temperature=g.get("temperature", 1.0), top_k=g.get("top_k", 50),
                            top_p=g.get("top_p", 1.0), penalty=g.get("repetition_penalty", 1.0), prompt_ids=kw["input_ids"].cpu().numpy(),
                            prompt_div=fanout, gen_ids=gen, n_gen=n, eos=(kw["eos_token_id"],), pad=kw["pad_token_id"], seed=g["seed"], call=9,
                            step=n, unfinished=unf, finish_step=fin)
        out = dict(tok=gen[:, n], logp=lp[:, n], unfinished=ref["unfinished"], finish_step=ref["finish_step"], kept=None)
        fails, w, waived = SR.check_sample(out, ref)
        assert fails == [] and waived == 0, (n, fails, waived)
        worst = max(worst, w)
        unf, fin = ref["unfinished"], ref["finish_step"]
    print(f"[sample] host replay of {rows} rows x {new} tokens: worst logp err/bound {worst:.3f}")
    return ids, gen


@pytest.mark.parametrize("cache", [True, False])
def test_tokens_and_logprobs_replay_on_the_host(small, monkeypatch, cache):
    cfg, model, kw = small
    ids, gen = replay_on_host(model, kw, monkeypatch, do_sample=True, temperature=0.8, top_k=20, top_p=0.9, repetition_penalty=1.3, seed=77,
                              use_cache=cache)
    # an eos in the middle: the first row's second token ends it, and the replay follows the flags
    replay_on_host(model, dict(kw, eos_token_id=int(gen[0, 1])), monkeypatch, do_sample=True, temperature=0.8, top_k=20, top_p=0.9,
                   repetition_penalty=1.3, seed=77, use_cache=cache, sync_every=100)


def test_num_return_sequences_reads_the_prompt_through_prompt_div(small, monkeypatch):
    from vlrlhf import _hip
    import vlrlhf.models.Llava as LL
    cfg, model, kw = small
    seen = []
    call = _hip.call
    monkeypatch.setattr(LL._hip, "call", lambda nm, *a: (seen.append((nm, a)) if nm == "vlr_sample_tokens" else None, call(nm, *a))[1])
    model._sampler_calls = 9
    model.generate(sampler="device", do_sample=True, num_return_sequences=3, max_new_tokens=2, seed=5, repetition_penalty=1.3, **kw)
    monkeypatch.undo()
    P, T = kw["input_ids"].shape
    a = seen[0][1]
    assert a[1] == 3 * P and a[9].shape == (P, T) and (a[10], a[11], a[12]) == (T, T, 3)      # one copy of the prompts, prompt_div = 3
    ids, gen = replay_on_host(model, kw, monkeypatch, fanout=3, do_sample=True, temperature=1.5, top_k=0, repetition_penalty=1.3, seed=5)
    assert any(len({tuple(gen[3 * p + j]) for j in range(3)}) > 1 for p in range(P)), "the samples of at least one prompt differ"
    for p in range(P):
        assert torch.equal(ids[3 * p:3 * p + 3, :T], kw["input_ids"][p].expand(3, T))


def test_generation_config_reaches_the_kernel_and_default_never_launches_it(small, monkeypatch):
    from vlrlhf import _hip
    import vlrlhf.models.Llava as LL
    cfg, model, kw = small
    seen, names = [], []
    call = _hip.call

    def spy(nm, *a):
        names.append(nm)
        if nm == "vlr_sample_tokens":
            seen.append(a)
        return call(nm, *a)
    monkeypatch.setattr(LL._hip, "call", spy)
    picks = []
    multinomial = torch.multinomial
    monkeypatch.setattr(torch, "multinomial", lambda *a, **k: (picks.append(1), multinomial(*a, **k))[1])
    # Qwen-VL-Chat's own settings, which the torch path replaces by top_k 50 / top_p 1
    gc = SimpleNamespace(do_sample=True, temperature=0.9, top_k=0, top_p=0.3, repetition_penalty=1.1, max_new_tokens=3, sampler="device")
    model.generate(generation_config=gc, **kw)
    assert len(seen) == 3 and picks == []
    for n, a in enumerate(seen):
        assert a[4] == 1 and (a[5], a[6], a[7], a[8]) == (0.9, 0, 0.3, 1.1) and a[15] == n and a[21] == n, a[4:9]
    model.generate(generation_config=gc, top_k=7, top_p=1.0, **kw)            # the keyword wins
    assert (seen[-1][6], seen[-1][7]) == (7, 1.0)
    # the default: the torch ops, and not one launch of the new kernel on either route
    seen.clear(), names.clear()
    gc.sampler = None
    for cache in (True, False):
        model.generate(generation_config=gc, use_cache=cache, **kw)
    assert seen == [] and "vlr_sample_tokens" not in names and len(picks) == 6


def test_grpo_with_device_sampler_resumes_to_the_same_bits(gpu, tmp_path):
    """vlrlhf.grpo.main --device_sampler true, two batches; a run resumed from the first checkpoint draws under the restored call word and
    lands on the uninterrupted run's weights"""
    import json
    from tests.golden_util import write_tiny_checkpoint
    from tests.test_hip_grpo import _grpo_args, _reward
    from vlrlhf import grpo
    ckpt, out = str(tmp_path / "ckpt"), str(tmp_path / "out")
    write_tiny_checkpoint(ckpt)
    seen = []

    def reward(q, r):
        seen.append(list(r))
        return _reward(q, r)
    tr = grpo.main(_grpo_args(ckpt, out, device_sampler=True), reward_fn=reward)
    torch.cuda.synchronize()
    assert tr.state.global_step == 2 and tr.model._sampler_calls == 2
    state = json.load(open(os.path.join(out, "checkpoint-1", "trainer_state.json")))
    assert state["sampler_calls"] == 1
    final_flat, second = tr.model.engine.policy.flat.clone(), seen[1]
    del tr
    seen.clear()
    tr2 = grpo.main(_grpo_args(ckpt, str(tmp_path / "out2"), device_sampler=True, resume_from_checkpoint=os.path.join(out, "checkpoint-1"),
                               save_steps=0), reward_fn=reward)
    torch.cuda.synchronize()
    assert tr2.state.global_step == 2 and tr2.model._sampler_calls == 2
    assert seen == [second]                                     # the same responses were drawn
    assert torch.equal(tr2.model.engine.policy.flat, final_flat)
