"""Host side of a trainable CLIP vision tower (--freeze_vision_tower False): the layout of its tensors in the trainable flat buffer,
the loader's rules per model family, and the argument parsers.  No GPU."""
import json
from types import SimpleNamespace

import pytest
import torch

from oracle import llava_dpo_oracle as O
from vlrlhf.engine import ParamLayout, WeightSet
from vlrlhf.utils import auto_load

CFG = dict(vit_hidden=128, vit_mlp=256, vit_layers=3, vit_heads=2, image_size=56, patch_size=14, hidden=256, inter=512, layers=2, heads=2,
           vocab=512, image_token=500, model_pad_token_id=501)
VT = "vision_tower."


def _unevaluated(W, cfg):
    last = cfg["vit_layers"] - 1
    return {k for k in W if k.startswith(VT) and (f"encoder.layers.{last}." in k or "post_layernorm" in k)}


@pytest.mark.parametrize("extra", [{}, dict(image_grid_pinpoints=[[56, 112]], kv_heads=1)], ids=["llava", "llavanext"])
def test_tower_entries_are_the_oracles_trainable_names_minus_the_unevaluated(extra):
    cfg = dict(CFG, **extra)
    W = O.random_weights(cfg, seed=1)
    if extra:
        W["image_newline"] = torch.zeros(cfg["hidden"])
    frozen, train = ParamLayout(cfg), ParamLayout(dict(cfg, train_vision_tower=True))
    names_f, names_t = {h for h, _, _, _ in frozen.hf_names()}, {h for h, _, _, _ in train.hf_names()}
    assert names_f == set(O.trainable_names(W))
    assert names_t == set(O.trainable_names(W, freeze_vision_tower=False)) - _unevaluated(W, cfg)
    # the frozen layout is a prefix-preserving subset: every decoder / projector entry keeps its place in its region's order
    order = [n for n, _, _ in train.entries if not n.startswith("vit.")]
    assert order == [n for n, _, _ in frozen.entries]
    # decay split = HF's grouping; the tower's matrices close the decay region (the last DDP bucket), its norms and biases the other
    for hf, name, r0, rows in train.hf_names():
        assert (train.offset[name] >= train.n_decay) == O.is_no_decay(hf), hf
    decay = [n for n, _, _ in train.entries[:train.n_decay_entries]]
    assert decay[-1] == "vit.patch_w" and decay[-3:] == ["vit.pos", "vit.cls", "vit.patch_w"]
    first = decay.index(next(n for n in decay if n.startswith("vit.")))
    assert all(n.startswith("vit.") for n in decay[first:]) and decay[first - 1] == "embed"
    assert train.bucket_after["tail"][1] == train.n_opt == train.numel
    assert all(train.offset[n] % 8 == 0 for n in train.offset)


def test_weightset_round_trips_the_fused_and_padded_tower_tensors():
    cfg = dict(CFG, train_vision_tower=True)
    W = O.random_weights(CFG, seed=2)
    ws = WeightSet(ParamLayout(cfg), "cpu")
    ws.load_state_dict(W)
    sd = ws.state_dict()
    for k in sd:
        assert sd[k].shape == W[k].shape and torch.equal(sd[k], W[k].bfloat16()), k
    pw = ws.v["vit.patch_w"]
    assert pw.shape == (128, 592) and float(pw[:, 588:].abs().max()) == 0.0          # K padded to a multiple of 8, padding zero
    # views, not copies: a write through the state dict lands in the flat buffer (named_parameters / .grad rely on it)
    name = VT + "vision_model.embeddings.patch_embedding.weight"
    sd[name][3, 1, 2, 5] = 7.0
    assert float(pw[3, 1 * 196 + 2 * 14 + 5]) == 7.0
    q = VT + "vision_model.encoder.layers.1.self_attn.k_proj.bias"
    sd[q][4] = 5.0
    assert float(ws.v["vit.l1.bqkv"][128 + 4]) == 5.0


@pytest.mark.parametrize("family", ["qwen_vl", "internlm_xc2"])
def test_layout_refuses_the_other_families(family):
    with pytest.raises(NotImplementedError, match="Qwen-VL" if family == "qwen_vl" else "InternLM-XComposer2"):
        ParamLayout(dict(CFG, family=family, train_vision_tower=True))


def _ckpt(tmp_path, arch):
    (tmp_path / "config.json").write_text(json.dumps(dict(architectures=[arch])))
    return str(tmp_path)


def _load(monkeypatch, path, use_lora, freeze):
    calls = []

    class Fake:
        config = SimpleNamespace()
        default_lora_target = ["q_proj"]

        def freeze_vision_tower(self):
            calls.append("freeze")

    def from_pretrained(p, *a, **k):
        calls.append(("load", k))
        return Fake()

    monkeypatch.setattr(auto_load.MyAutoModel, "from_pretrained", staticmethod(from_pretrained))
    sa = SimpleNamespace(model_name_or_path=path, freeze_vision_tower=freeze, label_pad_token_id=-100)
    ta = SimpleNamespace(use_lora=use_lora, seed=0)
    la = SimpleNamespace(q_lora=False, bits=4, lora_target_modules=None, lora_r=8, lora_alpha=16, lora_dropout=0.0, lora_bias="none", modules_to_save=None)
    auto_load.auto_load_rlmodel(sa, ta, la)
    return calls


@pytest.mark.parametrize("arch", ["LlavaForConditionalGeneration", "LlavaNextForConditionalGeneration"])
def test_loader_accepts_llava_and_llavanext(monkeypatch, tmp_path, arch):
    path = _ckpt(tmp_path, arch)
    assert _load(monkeypatch, path, False, False) == [("load", dict(train_vision_tower=True))]          # and freeze_vision_tower() is not called
    assert _load(monkeypatch, path, False, True) == [("load", {}), "freeze"]                              # the default: the parent's calls


def test_loader_with_lora_is_a_logged_noop(monkeypatch, tmp_path, capsys):
    path = _ckpt(tmp_path, "LlavaForConditionalGeneration")
    assert _load(monkeypatch, path, True, False) == [("load", {}), "freeze"]
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "freeze_vision_tower False" in out and "stays frozen" in out


@pytest.mark.parametrize("arch,name", [("QWenLMHeadModel", "QwenVL"), ("InternLMXComposer2ForCausalLM", "InternLMXC2")])
def test_loader_refuses_the_other_families_by_name(monkeypatch, tmp_path, arch, name):
    with pytest.raises(NotImplementedError, match=name):
        _load(monkeypatch, _ckpt(tmp_path, arch), False, False)


@pytest.mark.parametrize("mod", ["dpo", "sft"])
def test_entry_points_parse_the_flag(mod):
    import importlib
    m = importlib.import_module(f"vlrlhf.{mod}")
    for argv, want in (([], True), (["--freeze_vision_tower", "False"], False), (["--freeze_vision_tower", "True"], True)):
        script_args = m._parse(m.ScriptArguments, m.TrainingArguments, m.LoraArguments, argv=argv)[0]
        assert script_args.freeze_vision_tower is want
