"""CPU-only checks of the device sampler's plumbing: the entry point is exported and declared (ABI version unchanged), generate's keyword
rules (the ValueErrors, keyword wins over generation_config, a call without the new keywords builds today's argument list), the trainers'
device_sampler switch and the call counter's round trip through the PPO / GRPO checkpoint state."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from tests.test_decode_shared_host import StubModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_exported_declared_and_additive():
    from vlrlhf import _hip
    l = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "vlr.h")).read()
    assert hasattr(l, "vlr_sample_tokens") and "vlr_sample_tokens" in _hip.exported_symbols()
    assert _hip.helper("vlr_abi_version") == 9               # additive: no caller breaks
    proto = re.search(r"\bint vlr_sample_tokens\s*\(([^;{]*?)\)\s*;", hdr, re.S).group(1)
    assert len(_hip._SIGS["vlr_sample_tokens"]) == len([a for a in proto.split(",") if a.strip()]) == 31
    import sys
    sys.path.insert(0, os.path.join(ROOT, "vl-rlhf_amd"))
    import build_hip
    assert "sample.hip" in build_hip.SOURCES


def test_argument_ranges_are_refused_before_any_launch():
    from vlrlhf import _hip
    l = _hip.lib()
    one = 16                                                  # a non-null, aligned stand-in pointer: the checks never read it

    def call(B=2, V=8, ld=8, T=1.0, k=0, p=1.0, pen=1.0, logits=one, n_eos=0, step=0, out_ld=4, prompt=None, nT=0):
        return l.vlr_sample_tokens(logits, B, V, ld, 1, T, k, p, pen, prompt, nT, nT, 1, None, 0, 0, one if n_eos else None, n_eos, 0, 1, 0,
                                   step, None, one, one, one, out_ld, one, one, None, None)

    for kw, msg in ((dict(logits=None), b"null operand"), (dict(V=0), b"bad shape"), (dict(ld=7), b"bad shape"), (dict(B=0), b"bad shape"),
                    (dict(T=0.0), b"temperature 0"), (dict(T=-1.0), b"temperature -1"), (dict(p=0.0), b"top_p 0"), (dict(p=1.5), b"top_p 1.5"),
                    (dict(pen=0.0), b"repetition_penalty 0"), (dict(n_eos=9), b"n_eos 9"), (dict(step=4), b"step 4"),
                    (dict(pen=1.2, nT=3), b"null prompt_ids"), (dict(pen=1.2, V=(1 << 19) + 1, ld=1 << 20), b"repetition_penalty needs V")):
        assert call(**kw) == 1, kw
        assert l.vlr_last_error().startswith(b"vlr_sample_tokens: " + msg), (kw, l.vlr_last_error())


def _gen(m, **kw):
    from vlrlhf.models.Llava import LlavaForRL
    return LlavaForRL.generate(m, input_ids=torch.zeros(2, 4, dtype=torch.long), max_new_tokens=2, **kw)


def test_default_call_is_todays_call():
    """no new keyword: the positional arguments and keywords _generate_cached sees are the parent's (temperature 1, top_k 50, top_p 1, no
    `sampler`), whatever warper settings a generation_config carries - the torch path never read them"""
    seen = []

    class Rec(StubModel):
        def _generate_cached(self, ids, *a, **k):
            seen.append((a, k))
            return ids

    m = Rec()
    _gen(m, do_sample=True)
    _gen(m, do_sample=True, generation_config=SimpleNamespace(temperature=0.3, top_k=7, top_p=0.5, repetition_penalty=1.3, max_new_tokens=2))
    for a, k in seen:
        assert k == {} and a[2:6] == (True, 1.0, 50, 1.0) and a[6] == 0 and a[7] == {2} and a[8] is None, (a, k)
    assert not hasattr(m, "_sampler_calls")
    _gen(m, do_sample=True, temperature=0.7, top_k=5, top_p=0.9, sampler="torch")
    assert seen[-1][0][3:6] == (0.7, 5, 0.9) and seen[-1][1] == {}


def test_device_sampler_keyword_rules():
    from vlrlhf.models.Llava import DeviceSampler
    m = StubModel()
    for kw, name in ((dict(repetition_penalty=1.2), "repetition_penalty"), (dict(output_logprobs=True), "output_logprobs"), (dict(seed=3), "seed")):
        with pytest.raises(ValueError, match=f'{name} needs sampler="device"'):
            _gen(m, do_sample=True, **kw)
    _gen(m, do_sample=True, repetition_penalty=1.0)            # 1 is no penalty: the torch path takes it
    with pytest.raises(ValueError, match='"torch" or "device"'):
        _gen(m, sampler="cuda")
    with pytest.raises(ValueError, match=r"`temperature` \(=0\) has to be a strictly positive float"):
        _gen(m, sampler="device", do_sample=True, temperature=0)
    for p in (0, 1.5):
        with pytest.raises(ValueError, match=f"`top_p` has to be a float > 0 and < 1, but is {p}"):
            _gen(m, sampler="device", do_sample=True, top_p=p)
    with pytest.raises(ValueError, match="`penalty` has to be a strictly positive float, but is -1"):
        _gen(m, sampler="device", repetition_penalty=-1)
    with pytest.raises(ValueError, match="at most 8 eos ids"):
        _gen(m, sampler="device", eos_token_id=list(range(9)))
    m.seen.clear()
    # the generation config is read for what the keywords leave open; a keyword wins
    gc = SimpleNamespace(temperature=0.3, top_k=0, top_p=0.5, repetition_penalty=1.005, max_new_tokens=2, do_sample=True, sampler="device")
    _gen(m, generation_config=gc)
    ds = m.seen[-1]["sampler"]
    assert isinstance(ds, DeviceSampler) and ds.warp == (1, 0.3, 0, 0.5, 1.005)
    _gen(m, generation_config=gc, temperature=0.9, top_k=11, repetition_penalty=1.0, sampler="device")
    assert m.seen[-1]["sampler"].warp == (1, 0.9, 11, 0.5, 1.0)
    _gen(m, sampler="device")                                  # greedy, no config: the defaults
    ds = m.seen[-1]["sampler"]
    assert ds.warp == (0, 1.0, 50, 1.0, 1.0) and (ds.rows, ds.T0, ds.max_new, ds.div, ds.sync_every) == (2, 4, 2, 1, 8)
    assert m._sampler_calls == 3 and [c["sampler"].call for c in m.seen[-3:]] == [0, 1, 2]      # one bump per call
    # seed: the keyword, else the generator's initial seed, else torch's
    g = torch.Generator().manual_seed(1234)
    _gen(m, sampler="device", generator=g)
    assert m.seen[-1]["sampler"].seed == 1234
    _gen(m, sampler="device", generator=g, seed=77)
    assert m.seen[-1]["sampler"].seed == 77
    torch.manual_seed(4321)
    _gen(m, sampler="device")
    assert m.seen[-1]["sampler"].seed == 4321
    # the fan-out reads the prompt through prompt_div on the cached route: one copy of the prompt rows
    _gen(m, sampler="device", do_sample=True, num_return_sequences=3)
    ds = m.seen[-1]["sampler"]
    assert m.seen[-1]["fanout"] == 3 and (ds.rows, ds.div) == (6, 3) and ds.prompt.shape == (2, 4) and ds.full.shape == (6, 6)
    # nothing to generate: the ids (and no log-probs)
    from vlrlhf.models.Llava import LlavaForRL
    ids, lp = LlavaForRL.generate(m, input_ids=torch.zeros(2, 4, dtype=torch.long), max_length=4, sampler="device", output_logprobs=True)
    assert ids.shape == (2, 4) and lp.shape == (2, 0)


def test_device_sampler_trims_like_the_per_token_check():
    """result(): all rows finished -> the columns up to the last finish step, whatever was generated past it while nobody looked"""
    from vlrlhf.models.Llava import DeviceSampler
    ds = DeviceSampler(torch.ones(3, 2, dtype=torch.long), 1, 2 + 9, True, 1.0, 50, 1.0, 1.0, {2}, 0, 1, 0, sync_every=4)
    ds.n = 8                                                   # two host looks; the rows finished at steps 1, 4 and 2
    ds.unfinished.zero_()
    ds.finish.copy_(torch.tensor([1, 4, 2], dtype=torch.int32))
    ds.full[:, 2:] = 7
    ids, lp = ds.result(True)
    assert ids.shape == (3, 2 + 5) and lp.shape == (3, 5)
    ds.unfinished[1] = 1                                       # one row still running: everything generated so far
    assert ds.result().shape == (3, 2 + 8)
    assert not ds.done()
    ds.n = 9
    assert ds.done()


def test_config_switch_cli_and_checkpoint_state():
    from vlrlhf import grpo, ppo
    from vlrlhf.base.trainer import GRPOConfig, PPOConfig, VLGRPOTrainer, VLPPOTrainer
    assert PPOConfig().device_sampler is False and GRPOConfig(batch_size=1, num_generations=2, mini_batch_size=2).device_sampler is False
    _, cfg, _ = grpo._parse(["--batch_size", "1", "--num_generations", "2", "--mini_batch_size", "2", "--device_sampler", "true"])
    assert cfg.device_sampler is True
    _, cfg, _ = ppo._parse(["--batch_size", "2", "--mini_batch_size", "2", "--device_sampler", "true"])
    assert cfg.device_sampler is True
    _, cfg, _ = ppo._parse(["--batch_size", "2", "--mini_batch_size", "2"])
    assert cfg.device_sampler is False
    gen = torch.Generator().manual_seed(5)
    for cls, extra in ((VLGRPOTrainer, dict(_sample_gen=gen)), (VLPPOTrainer, dict(_perm_gen=gen, kl_ctl=SimpleNamespace(value=0.2), is_peft_model=True))):
        inner = SimpleNamespace(_sampler_calls=7)
        model = inner if cls is VLGRPOTrainer else SimpleNamespace(pretrained_model=inner)
        me = SimpleNamespace(config=SimpleNamespace(device_sampler=True, seed=10, num_generations=2), model=model, **extra)
        for name in ("_sampling_model", "_sampler_state", "_restore_sampler_state", "_device_sampler_kwargs"):
            setattr(me, name, getattr(cls, name).__get__(me))
        state = cls._checkpoint_extra(me)
        assert state["sampler_calls"] == 7
        inner._sampler_calls = 0
        cls._restore_extra(me, state, "unused")
        assert inner._sampler_calls == 7                       # a resumed run draws under the call word the interrupted one would have
        assert me._device_sampler_kwargs({}) == dict(sampler="device", seed=12)
        assert me._device_sampler_kwargs(dict(seed=1, sampler="torch")) == dict(seed=1, sampler="torch")      # the caller's keywords win
        me.config.device_sampler = False
        assert "sampler_calls" not in cls._checkpoint_extra(me) and me._device_sampler_kwargs({}) == {}
