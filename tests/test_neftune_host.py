"""CPU-only checks of NEFTune (neftune_noise_alpha): the numpy replay of the noise generator (tests/neftune_ref.py) against known answers
and against the moments of U(-m, m), and the trainer / argument / checkpoint plumbing over a recording stand-in for the engine."""
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import neftune_ref as R
from tests.golden_util import TINY_PROCESSOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------- the generator
def test_philox_replay_matches_known_answers():
    """Philox4x32-10 known answers.  The first and the last are the Random123 kat_vectors entries for an all-zero and an all-ones
    counter and key; the middle one has a mixed counter and key.  The Random123 file itself is not at hand: all three were confirmed
    against an independent implementation instead, PyTorch's at::philox_engine (ATen/core/PhiloxRNGEngine.h: seed = key, offset =
    counter words 0-1, subsequence = counter words 2-3), compiled for the host."""
    hexs = lambda w: [f"{int(x):08x}" for x in w]      # noqa: E731
    assert hexs(R.philox4x32_10(0, 0, 0, 0, 0, 0)) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    assert hexs(R.philox4x32_10(3, 0, 7, 0, 0x12345678, 0xDEADBEEF)) == ["28652a93", "6c6a7b87", "12ee3bad", "6042f021"]
    f = 0xFFFFFFFF
    assert hexs(R.philox4x32_10(f, f, f, f, f, f)) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    # the arguments broadcast, and a block is a function of its own counter only
    w = R.philox4x32_10(np.arange(5).reshape(1, 5), np.arange(3).reshape(3, 1), 7, 0, 1, 2)
    assert all(x.shape == (3, 5) and x.dtype == np.uint32 for x in w)
    one = R.philox4x32_10(4, 2, 7, 0, 1, 2)
    assert [int(x[2, 4]) for x in w] == [int(x) for x in one]
    # column c of a row = word c % 4 of block c / 4
    words = R.noise_words([2], 24, (2 << 32) | 1, 7, 0)
    assert words.shape == (1, 24) and [int(v) for v in words[0, 16:20]] == [int(x) for x in one]


N = 1 << 20


@pytest.fixture(scope="module")
def draws():
    """N = 2^20 replayed values at m = 1 (scale = 2^-23): 256 tokens x 4096 columns, for (call, pass) = (1, 0), (2, 0), (1, 1)"""
    key = (3 << 32) | 42
    return {cp: R.noise(np.arange(256), 4096, 2.0 ** -23, key, *cp).reshape(-1).astype(np.float64) for cp in ((1, 0), (2, 0), (1, 1))}


def test_noise_is_uniform_on_the_open_interval(draws):
    """moments of U(-1, 1), each at 6 sigma of its own estimator over N independent draws: mean (variance 1/3 -> sigma = 1/sqrt(3N)),
    variance (var of x^2 = 1/5 - 1/9 = 4/45 -> sigma = sqrt(4/45)/sqrt(N)), 16 equal bins (binomial(N, 1/16))"""
    n = draws[(1, 0)]
    assert n.size == N
    assert np.all(np.abs(n) < 1.0) and np.all(n != 0.0)
    mean, var = float(n.mean()), float(n.var())
    print(f"mean {mean:.3e} (bound {6 / math.sqrt(3 * N):.3e})  var - 1/3 {var - 1 / 3:.3e} (bound {6 * math.sqrt(4 / 45) / math.sqrt(N):.3e})")
    assert abs(mean) <= 6 / math.sqrt(3 * N)
    assert abs(var - 1 / 3) <= 6 * math.sqrt(4 / 45) / math.sqrt(N)
    counts = np.histogram(n, bins=16, range=(-1.0, 1.0))[0]
    sigma = math.sqrt(N * (1 / 16) * (15 / 16))
    print("bins", (counts - N / 16).tolist(), f"bound {6 * sigma:.1f}")
    assert counts.sum() == N and np.all(np.abs(counts - N / 16) <= 6 * sigma)
    # symmetric by construction: the 2^24 values h = r - 8388607.5 come in +- pairs (r <-> 2^24 - 1 - r)
    r = np.array([0, 1, 8388607, 8388608, (1 << 24) - 2, (1 << 24) - 1], dtype=np.float32) - np.float32(8388607.5)
    assert (r == -r[::-1]).all() and r[2] == -0.5 and r[3] == 0.5 and r[-1] == 8388607.5


def test_streams_of_different_calls_and_passes_are_uncorrelated(draws):
    """sample correlation of two independent streams: sigma = 1/sqrt(N), checked at 6 sigma"""
    a = draws[(1, 0)]
    for other in ((2, 0), (1, 1)):
        c = float(np.corrcoef(a, draws[other])[0, 1])
        print(f"correlation (1, 0) vs {other}: {c:.3e} (bound {6 / math.sqrt(N):.3e})")
        assert abs(c) <= 6 / math.sqrt(N)
        assert not np.array_equal(a, draws[other])


def test_magnitude_follows_the_reference_rule():
    """m = alpha / sqrt(T * H) of the hook, scale = m 2^-23 exactly; |n| < m and n != 0 at a real shape as well"""
    from vlrlhf.engine import neftune_scale
    m, scale = neftune_scale(5.0, 640, 4096)
    assert m == float(np.float32(5.0 / math.sqrt(640 * 4096))) and scale == m * 2.0 ** -23
    assert float(np.float32(scale)) == scale
    n = R.noise(np.arange(64), 4096, scale, 42, 1, 0)
    assert n.dtype == np.float32 and np.all(np.abs(n) < np.float32(m)) and np.all(n != 0)
    assert float(np.abs(n).max()) > 0.999 * m                                   # ... and it fills the interval
    assert not R.noise([0], 8, 0.0, 42, 1, 0).any()                              # scale 0: no noise
    # bf16 rounding of the replay: nearest, ties to even
    f = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-5], dtype=np.float32)      # 1 + 2^-8 (tie -> 1), 1 + 3 2^-8 (tie -> 1 + 2^-6)
    assert R.bf16_bits(f).tolist() == torch.from_numpy(f).bfloat16().view(torch.int16).numpy().view(np.uint16).tolist()


def test_replay_touches_text_rows_only():
    src = np.array([[0, -1, -2, 1, 2], [-(2 ** 31), 0, 1, -3, 2]], dtype=np.int64)
    x = torch.arange(2 * 5 * 8, dtype=torch.float32).reshape(10, 8)
    nf = (42, 1, 0, 3, 2.0 ** -23)
    y = R.add_noise(x, src, 3, nf)
    text = (src.reshape(-1) >= 0)
    assert torch.equal(y[~torch.from_numpy(text)], x[~torch.from_numpy(text)]) and (y[torch.from_numpy(text)] != x[torch.from_numpy(text)]).all()
    # row (b, s) draws the stream of its PRE-merge token b * T + t, wherever the merge put it
    assert np.array_equal(y[7].numpy(), x[7].numpy() + R.noise([1 * 3 + 1], 8, nf[4], 42, 1, 0)[0])          # row (1, 2) holds token t = 1
    yb = R.add_noise(x.bfloat16(), src, 3, nf)
    assert yb.dtype == torch.bfloat16 and torch.equal(yb[1], x.bfloat16()[1])


# ---------------------------------------------------------------------------------------------------------- trainers
class _Engine:
    """what the trainers touch of the engine around NEFTune and checkpoints"""

    def __init__(self):
        self.neftune, self._neftune_calls, self.opt_step, self.log = None, 0, 0, []
        self.dev = torch.device("cpu")
        self.policy = SimpleNamespace(load_state_dict=lambda sd: None)

    def set_neftune(self, alpha, seed=42, rank=0):
        self.log.append((alpha, seed, rank))
        self.neftune = None if alpha is None else dict(alpha=alpha, seed=seed, rank=rank)

    def optimizer_state(self):
        return None


def _model():
    return SimpleNamespace(engine=_Engine(), save_pretrained=lambda path: None)


def _sft(model, args=None, **kw):
    from vlrlhf.models.Llava import LlavaProcessor, LlavaSFTTRainer
    proc = LlavaProcessor(TINY_PROCESSOR)
    proc.train()
    return LlavaSFTTRainer(model=model, args=args if args is not None else SimpleNamespace(), processor=proc, max_seq_length=64, **kw)


def _dpo(model, args):
    from vlrlhf.base.trainer import VLDPOTrainer
    return VLDPOTrainer(model, None, 0.1, 0, "sigmoid", args, None, -100, 0, precompute_ref_log_probs=False, reference_free=True)


def test_argument_fields_parse():
    from vlrlhf import dpo, sft
    for mod in (dpo, sft):
        _, t, _ = dpo._parse(mod.ScriptArguments, mod.TrainingArguments, mod.LoraArguments, argv=["--neftune_noise_alpha", "5"])
        assert t.neftune_noise_alpha == 5.0 and isinstance(t.neftune_noise_alpha, float)
        _, t, _ = dpo._parse(mod.ScriptArguments, mod.TrainingArguments, mod.LoraArguments, argv=[])
        assert t.neftune_noise_alpha is None and t.seed == 42


def test_trainers_accept_alpha_from_the_constructor_and_from_args():
    """fails before the feature: VLSFTTrainer raised NotImplementedError for every model, VLDPOTrainer ignored the field"""
    a = _sft(_model(), neftune_noise_alpha=5.0)
    b = _sft(_model(), args=SimpleNamespace(neftune_noise_alpha=5.0))
    c = _dpo(_model(), SimpleNamespace(neftune_noise_alpha=5))
    assert a.neftune_noise_alpha == b.neftune_noise_alpha == c.neftune_noise_alpha == 5.0
    assert _sft(_model(), args=SimpleNamespace(neftune_noise_alpha=5.0), neftune_noise_alpha=2.0).neftune_noise_alpha == 2.0      # trl: the argument wins
    assert _sft(_model()).neftune_noise_alpha is None and _dpo(_model(), SimpleNamespace()).neftune_noise_alpha is None
    assert all(t.model.engine.log == [] for t in (a, b, c)), "constructing a trainer must not switch the noise on"


def test_wrappers_without_support_are_refused():
    for model in (SimpleNamespace(engine=None), SimpleNamespace(engine=SimpleNamespace()), SimpleNamespace()):
        with pytest.raises(NotImplementedError, match="neftune"):
            _sft(model, neftune_noise_alpha=5.0)
        with pytest.raises(NotImplementedError, match="neftune"):
            _sft(model, args=SimpleNamespace(neftune_noise_alpha=5.0))
        with pytest.raises(NotImplementedError, match="neftune"):
            _dpo(model, SimpleNamespace(neftune_noise_alpha=5.0))
    assert _sft(SimpleNamespace(engine=None)).neftune_noise_alpha is None          # without alpha such a wrapper is fine


@pytest.mark.parametrize("make", [lambda m, a: _sft(m, args=a), _dpo], ids=["sft", "dpo"])
def test_noise_is_on_from_before_train_to_the_end_of_train(make):
    model = _model()
    eng = model.engine
    tr = make(model, SimpleNamespace(neftune_noise_alpha=5.0, seed=7))
    seen = []

    def loop(resume):
        seen.append(eng.neftune)                       # train() itself has not switched anything on yet
        tr._before_train()
        seen.append(eng.neftune)
        if resume == "boom":
            raise RuntimeError("boom")
        return "state"

    tr._train = loop
    assert tr.train() == "state"
    assert seen == [None, dict(alpha=5.0, seed=7, rank=0)] and eng.neftune is None
    assert eng.log == [(5.0, 7, 0), (None, 42, 0)]
    with pytest.raises(RuntimeError, match="boom"):          # a failed run switches it off too
        tr.train("boom")
    assert eng.neftune is None and eng.log[-1][0] is None
    # without alpha the engine is never touched
    quiet = make(_model(), SimpleNamespace())
    quiet._train = lambda resume: quiet._before_train()
    quiet.train()
    assert quiet.model.engine.log == []
    # seed default (transformers.TrainingArguments.seed = 42)
    d = make(_model(), SimpleNamespace(neftune_noise_alpha=1.0))
    d._before_train()
    assert d.model.engine.log == [(1.0, 42, 0)]


def test_engine_key_layout_and_counter():
    """set_neftune on the engine class itself (no GPU needed for the bookkeeping): seed in the low word, rank in the high word;
    switching off and on again keeps the call counter"""
    from vlrlhf.engine import LlavaHipEngine
    e = SimpleNamespace(neftune=None, _neftune_calls=11)
    LlavaHipEngine.set_neftune(e, 5, seed=42, rank=3)
    assert e.neftune == dict(alpha=5.0, key=(3 << 32) | 42)
    LlavaHipEngine.set_neftune(e, None)
    assert e.neftune is None and e._neftune_calls == 11
    LlavaHipEngine.set_neftune(e, 0.0, seed=-1, rank=0)
    assert e.neftune["key"] == 0xFFFFFFFF
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="neftune_noise_alpha"):
            LlavaHipEngine.set_neftune(e, bad)


def test_counter_round_trips_through_the_checkpoint(tmp_path):
    model = _model()
    tr = _sft(model, args=SimpleNamespace(neftune_noise_alpha=5.0, output_dir=str(tmp_path)))
    model.engine._neftune_calls = 7
    path = tr.save_checkpoint(2, 4, 0)
    assert json.load(open(os.path.join(path, "trainer_state.json")))["neftune_calls"] == 7
    model.engine._neftune_calls = 0
    tr.load_checkpoint(path)
    assert model.engine._neftune_calls == 7
    # a checkpoint written before the counter existed resumes at 0
    st = json.load(open(os.path.join(path, "trainer_state.json")))
    del st["neftune_calls"]
    json.dump(st, open(os.path.join(path, "trainer_state.json"), "w"))
    tr.load_checkpoint(path)
    assert model.engine._neftune_calls == 0


def test_entry_point_is_declared_bound_and_validates():
    """fails before the feature: the library has no vlr_neftune_add"""
    from vlrlhf import _hip
    l = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "vlr.h")).read()
    assert "vlr_neftune_add(" in hdr and hasattr(l, "vlr_neftune_add") and "vlr_neftune_add" in _hip.exported_symbols()
    assert _hip.helper("vlr_abi_version") == 9               # additive entry point: no caller breaks
    assert l.vlr_neftune_add(None, 0, None, 1, 8, 8, 8, 0.0, 0, 0, 0, None) == 1 and b"vlr_neftune_add: null argument" in l.vlr_last_error()
    # (validation comes before the launch: the made-up pointers are never followed)
    assert l.vlr_neftune_add(64, 0, 64, 1, 8, 8, 12, 0.0, 0, 0, 0, None) == 1 and b"H % 8" in l.vlr_last_error()
    assert l.vlr_neftune_add(64, 1, 64, 1, 8, 8, 8, 1.0, 0, 0, 0, None) == 1 and b"scale" in l.vlr_last_error()
