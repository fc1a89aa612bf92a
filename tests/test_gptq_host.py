"""GPTQ int4 base weights (q_lora), host side: the checkpoint format, the loader's fused re-layout, every refusal, and
auto_load_rlmodel's q_lora semantics.  No GPU: the packed tensors are read, validated and re-laid on the host (vlrlhf/gptq.py); the
kernels that consume them are tested in tests/test_hip_gptq.py."""
import json
import os
import types

import pytest
import torch

from tests import gptq_ref as R
from tests.golden_util import load_case


def rand_packed(K, N, g, seed=0):
    gen = torch.Generator().manual_seed(seed)
    G = K // R.group(K, g)
    q = torch.randint(0, 16, (K, N), generator=gen, dtype=torch.int32)
    zero = torch.randint(1, 17, (G, N), generator=gen, dtype=torch.int32)
    scales = (torch.rand(G, N, generator=gen) * 0.02 + 0.001).half()
    return q, zero, scales


def test_pack_dequant_is_exact_and_matches_the_package():
    from vlrlhf import gptq
    K, N, g = 128, 24, 32
    q, zero, scales = rand_packed(K, N, g)
    zero[0, 3] = 16                                            # stored 15
    t = R.pack(q, zero, scales, g)
    grp = torch.arange(K) // g
    want = (scales.float()[grp] * (q - zero[grp]).float()).to(torch.bfloat16).t()
    assert torch.equal(R.dequant(t["qweight"], t["qzeros"], t["scales"], g), want)
    assert torch.equal(gptq.dequant(t["qweight"], t["qzeros"], t["scales"], g), want)
    # stored zero 15 decodes to 16, without wrapping to 0
    assert int((t["qzeros"][0, 0].item() >> 12) & 15) == 15
    assert torch.equal(want[3, :g].float(), (scales[0, 3].float() * (q[:g, 3] - 16).float()).to(torch.bfloat16).float())
    # group_size -1 is one group over all of K
    q1, z1, s1 = rand_packed(K, N, -1, seed=1)
    t1 = R.pack(q1, z1, s1, -1)
    assert torch.equal(gptq.dequant(t1["qweight"], t1["qzeros"], t1["scales"], -1), R.dequant(t1["qweight"], t1["qzeros"], t1["scales"], -1))
    assert gptq.PackedLinear(t1["qweight"], t1["qzeros"], t1["scales"], -1).g == K


def test_known_answer_pins_the_nibble_order():
    """8 x 8, written by hand: q[k][n] = (k + 2 n) % 16, stored zero of column n = n, scale of column n = 2^-n"""
    from vlrlhf import gptq
    qweight = torch.zeros(1, 8, dtype=torch.int32)
    for n in range(8):
        word = 0
        for k in range(8):
            word |= ((k + 2 * n) % 16) << (4 * k)              # nibble k of the word of column n = row k
        qweight[0, n] = word - (1 << 32) if word >= 1 << 31 else word
    zword = 0
    for n in range(8):
        zword |= n << (4 * n)                                  # nibble n of the one qzeros word = column n
    qzeros = torch.tensor([[zword - (1 << 32) if zword >= 1 << 31 else zword]], dtype=torch.int32)
    scales = torch.tensor([[2.0 ** -n for n in range(8)]], dtype=torch.float16)
    want = torch.tensor([[(2.0 ** -n) * (((k + 2 * n) % 16) - (n + 1)) for k in range(8)] for n in range(8)])
    for fn in (R.dequant, gptq.dequant):
        assert torch.equal(fn(qweight, qzeros, scales, -1).float(), want), fn.__module__


def _layout_cfg(name):
    z, cfg, W, W_ref, batch, rows = load_case(name)
    if name == "qwenvl_small":
        cfg = dict(cfg, family="qwen_vl")
    return cfg, W


@pytest.mark.parametrize("name", ["llava_hipsmall", "qwenvl_small"])
def test_fused_relayout_is_the_bf16_loaders_row_order(name):
    """dequantising the loader's fused packed tensors on the host gives the tensors the bf16 loader builds from the dequantised
    checkpoint: q|k|v and gate|up stacked in the same order (Qwen-VL: one fused c_attn, gate = w2, up = w1)"""
    from vlrlhf import gptq
    from vlrlhf.engine import ParamLayout, WeightSet
    cfg, W = _layout_cfg(name)
    g = 32
    packed_sd, deq_sd = R.quantize_state_dict(W, g)
    lay_q, lay = ParamLayout(dict(cfg, gptq=dict(group_size=g))), ParamLayout(cfg)
    assert lay_q.packed and not lay.packed and lay_q.numel < lay.numel
    packed = gptq.load_packed_decoder(packed_sd, lay_q, g)
    ws = WeightSet(lay, "cpu")
    ws.load_state_dict(deq_sd, strict=False)
    assert sorted(packed) == sorted(n for n in lay.shape if gptq.is_packed_entry(n)) and len(packed) == 4 * cfg["layers"]
    for n, lin in packed.items():
        assert torch.equal(lin.dequant(), ws.v[n]), n
        assert torch.equal(R.dequant(lin.qweight, lin.qzeros, lin.scales, lin.g), ws.v[n]), n
    # everything that is not packed loads exactly as before, and no packed entry takes room in the flat buffer
    wq = WeightSet(lay_q, "cpu")
    wq.load_state_dict(packed_sd, strict=False)
    assert set(wq.v) == set(ws.v) - set(packed)
    for n in wq.v:
        assert torch.equal(wq.v[n], ws.v[n]), n
    if name == "qwenvl_small":
        assert any(n.endswith(".bqkv") for n in wq.v)          # the c_attn bias stays bf16


def _hf(**quant):
    return dict(architectures=["LlavaForConditionalGeneration"], quantization_config=dict(dict(quant_method="gptq", bits=4, group_size=32), **quant))


def test_refusals_of_the_format():
    from vlrlhf import gptq
    from vlrlhf.engine import ParamLayout
    assert gptq.parse_quantization_config(dict(architectures=["x"])) is None
    assert gptq.parse_quantization_config(_hf())["group_size"] == 32
    with pytest.raises(NotImplementedError, match="bits=8"):
        gptq.parse_quantization_config(_hf(bits=8))
    with pytest.raises(NotImplementedError, match="bits=3"):
        gptq.parse_quantization_config(_hf(bits=3))
    with pytest.raises(NotImplementedError, match="gptq_v2"):
        gptq.parse_quantization_config(_hf(checkpoint_format="gptq_v2"))
    with pytest.raises(NotImplementedError, match="quant_method"):
        gptq.parse_quantization_config(_hf(quant_method="awq"))
    cfg, W = _layout_cfg("llava_hipsmall")
    packed_sd, _ = R.quantize_state_dict(W, 32)
    lay = ParamLayout(dict(cfg, gptq=dict(group_size=32)))
    key = "language_model.model.layers.0.self_attn.k_proj.g_idx"
    bad = dict(packed_sd)
    bad[key] = packed_sd[key].flip(0).contiguous()             # act-order: a permuted g_idx
    with pytest.raises(NotImplementedError, match="g_idx"):
        gptq.load_packed_decoder(bad, lay, 32)
    for gs in (48, 16, 24):                                    # not a multiple of 32, or not a divisor of K
        with pytest.raises(ValueError, match="group_size"):
            gptq.group_size_for(256, gs)
    assert gptq.group_size_for(256, -1) == 256 and gptq.group_size_for(256, 64) == 64
    q, zero, scales = rand_packed(64, 12, 32)                  # N = 12 is no multiple of 8
    with pytest.raises(ValueError, match="multiple of 8"):
        gptq.PackedLinear(torch.zeros(8, 12, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32), scales, 32)
    missing = {k: v for k, v in packed_sd.items() if not k.endswith("layers.1.mlp.down_proj.qzeros")}
    with pytest.raises(KeyError, match="qzeros"):
        gptq.load_packed_decoder(missing, lay, 32)


def test_internlm_xcomposer2_keeps_its_own_refusal(tmp_path):
    from vlrlhf.models.InternLMXC2 import InternLMXC2ForRL
    with open(tmp_path / "config.json", "w") as f:
        json.dump(dict(architectures=["InternLMXComposer2ForCausalLM"], quantization_config=dict(quant_method="gptq", bits=4, group_size=128)), f)
    with pytest.raises(NotImplementedError, match="InternLM-XComposer2"):
        InternLMXC2ForRL.from_pretrained(str(tmp_path))


class _HostModel:
    """what auto_load_rlmodel touches of a model, built by the real host loader (the engine itself needs the GPU: the same call on the
    real model is in tests/test_hip_gptq.py)"""
    default_lora_target = ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]

    def __init__(self, path):
        from safetensors.torch import load_file
        from vlrlhf import gptq
        from vlrlhf.engine import ParamLayout
        from vlrlhf.models.Llava import _cfg_from_hf
        with open(os.path.join(path, "config.json")) as f:
            hf = json.load(f)
        cfg = _cfg_from_hf(hf)
        quant = gptq.parse_quantization_config(hf)
        self.packed = None
        if quant:
            cfg["gptq"] = quant
            self.packed = gptq.load_packed_decoder(load_file(os.path.join(path, "model.safetensors")), ParamLayout(cfg), quant["group_size"])
        self.config = types.SimpleNamespace()

    def freeze_vision_tower(self):
        pass


def _args(path, use_lora, q_lora, bits=4):
    return (types.SimpleNamespace(model_name_or_path=str(path), label_pad_token_id=-100, freeze_vision_tower=True),
            types.SimpleNamespace(use_lora=use_lora, seed=3),
            types.SimpleNamespace(q_lora=q_lora, bits=bits, lora_r=8, lora_alpha=16, lora_dropout=0.05, lora_target_modules="auto",
                                  lora_bias="none", modules_to_save=None))


def _write(tmp_path, name, g=32, quantised=True, **quant):
    from vlrlhf.models.Llava import _hf_from_cfg
    cfg, W = _layout_cfg("llava_hipsmall")
    path = str(tmp_path / name)
    if quantised:
        R.write_checkpoint(path, _hf_from_cfg(cfg), W, g, **quant)
    else:
        from safetensors.torch import save_file
        os.makedirs(path)
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(_hf_from_cfg(cfg), f)
        save_file({k: v.to(torch.bfloat16).contiguous() for k, v in W.items()}, os.path.join(path, "model.safetensors"))
    return path, cfg


def test_auto_load_rlmodel_q_lora(tmp_path, monkeypatch):
    """q_lora + use_lora on a written GPTQ checkpoint -> a packed model and the LoRA config (NotImplementedError before this feature);
    the two misuses are ValueErrors, other widths NotImplementedError"""
    from vlrlhf.utils import auto_load
    monkeypatch.setattr(auto_load.MyAutoModel, "from_pretrained", classmethod(lambda cls, path, *a, **k: _HostModel(path)))
    path, cfg = _write(tmp_path, "q")
    model, ref, lora = auto_load.auto_load_rlmodel(*_args(path, True, True))
    assert ref is None and model.packed is not None and len(model.packed) == 4 * cfg["layers"]
    assert lora["r"] == 8 and lora["lora_dropout"] == 0.05 and lora["seed"] == 3 and sorted(lora["target_modules"]) == sorted(model.default_lora_target)
    assert model.config.use_cache is False and model.config.label_pad_token_id == -100
    # a GPTQ checkpoint loads packed with --use_lora alone too (the reference's from_pretrained reads quantization_config itself)
    assert auto_load.auto_load_rlmodel(*_args(path, True, False))[0].packed is not None
    with pytest.raises(ValueError, match="cannot be trained"):
        auto_load.auto_load_rlmodel(*_args(path, False, False))
    with pytest.raises(NotImplementedError, match="bits 8"):
        auto_load.auto_load_rlmodel(*_args(path, True, True, bits=8))
    plain, _ = _write(tmp_path, "plain", quantised=False)
    with pytest.raises(ValueError, match="no quantization_config"):
        auto_load.auto_load_rlmodel(*_args(plain, True, True))
    assert auto_load.auto_load_rlmodel(*_args(plain, True, False))[0].packed is None
    for name, quant, word in (("b8", dict(bits=8), "bits=8"), ("v2", dict(checkpoint_format="gptq_v2"), "gptq_v2")):
        p, _ = _write(tmp_path, name, **quant)
        with pytest.raises(NotImplementedError, match=word):
            auto_load.auto_load_rlmodel(*_args(p, True, True))


def test_packed_model_refuses_merge_and_whole_model_save(tmp_path):
    """merge_and_unload and save_pretrained of a packed model raise, as peft does for GPTQ (checked on the methods themselves: a packed
    engine is all they look at)"""
    from vlrlhf.engine import LlavaHipEngine
    from vlrlhf.models.Llava import LlavaForRL
    eng = types.SimpleNamespace(packed={"l0.wqkv": None}, lora=dict(r=8, scale=2.0))
    eng.merged_weights = lambda: LlavaHipEngine.merged_weights(eng)
    model = types.SimpleNamespace(engine=eng, is_packed=True)
    with pytest.raises(NotImplementedError, match="GPTQ"):
        LlavaForRL.merge_and_unload(model)
    with pytest.raises(NotImplementedError, match="save_adapter"):
        LlavaForRL.save_pretrained(model, str(tmp_path / "out"))
    assert not os.path.exists(tmp_path / "out")
    assert LlavaForRL.is_packed.fget(types.SimpleNamespace(engine=types.SimpleNamespace(packed=None))) is False


def test_c_abi_declares_the_packed_entry_points():
    from vlrlhf import _hip
    l = _hip.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vlr.h")).read()
    for name in ("vlr_gptq_dequant_bf16", "vlr_gemv_w4", "vlr_gemv_w4_workspace_bytes", "vlr_decoder_layer_decode_w4"):
        assert name + "(" in hdr and hasattr(l, name) and name in _hip.exported_symbols(), name
    assert _hip.helper("vlr_abi_version") == 9
    assert l.vlr_gemv_w4_workspace_bytes(4, 4096, 4096) > 0
    FAKE = 1 << 20
    err = lambda rc, word: (rc == 1 and word in l.vlr_last_error().decode()) or pytest.fail(l.vlr_last_error().decode())  # noqa: E731
    err(l.vlr_gptq_dequant_bf16(FAKE, FAKE, FAKE, FAKE, 128, 60, 32, None), "multiples of 8")
    err(l.vlr_gptq_dequant_bf16(FAKE, FAKE, FAKE, FAKE, 128, 64, 48, None), "group_size")
    err(l.vlr_gptq_dequant_bf16(None, FAKE, FAKE, FAKE, 128, 64, 32, None), "null")
    w4 = lambda M, N, K, g: l.vlr_gemv_w4(0, FAKE, K, FAKE, FAKE, FAKE, g, FAKE, N, None, None, 0, None, None, None, 0, 128, 0, M, N, K, FAKE, None)  # noqa: E731
    err(w4(17, 64, 128, 32), "M = 17")
    err(w4(4, 60, 128, 32), "multiple of 8")
    err(w4(4, 64, 128, 96), "group_size")
