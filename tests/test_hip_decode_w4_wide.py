"""generate() over a packed GPTQ int4 base at 20 rows on the MI355X: the decode scratch is sized for 64-row groups, so every skinny GEMM
of a step - the four packed projections of each layer (vlr_gemv_wide_w4 / _lora inside vlr_decoder_layer_decode_w4 / _w4_lora) and the
bf16 lm-head - is one pass over its weights; withholding the wide scratch (engine.wide_gemv = False: 16-row groups, what the packed
route did before) must give the same tokens and the same logits at every step, bit for bit.  llava_hipsmall, packed as
tests/test_hip_gptq.py packs it (group 32).  Needs a real MI355X:  pytest -m gpu"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_hip_decode_lora import PEFT, Spy, wake_adapters  # noqa: E402
from tests.test_hip_gptq import llava_pair  # noqa: E402

ROWS, NEW = 20, 6


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return torch.device("cuda")


def decoder_scratch_need(eng, lora):
    """(bytes the packed decoder layer needs for 16-row groups, bytes from which it takes the 64-row groups) at ROWS rows"""
    from vlrlhf import _hip
    lib = _hip.lib()
    shapes = ((eng.Nqkv, eng.H), (eng.H, eng.Nq), (2 * eng.I, eng.H), (eng.H, eng.I))
    if lora:
        r = eng.lora["r"]
        rt = (eng.lora_layout.qkv_targets * r, r, 2 * r, r)
        return (max(int(lib.vlr_gemv_lora_workspace_bytes(16, n, k, t)) for (n, k), t in zip(shapes, rt)),
                max(int(lib.vlr_gemv_wide_lora_workspace_bytes(ROWS, n, k, t)) for (n, k), t in zip(shapes, rt)))
    return (max(int(lib.vlr_gemv_w4_workspace_bytes(16, n, k)) for n, k in shapes),
            max(int(lib.vlr_gemv_wide_w4_workspace_bytes(ROWS, n, k)) for n, k in shapes))


@pytest.mark.parametrize("lora", [False, True])
def test_twenty_rows_over_packed_weights_wide_equals_16_row_groups(gpu, tmp_path, monkeypatch, lora):
    cfg, batch, A, _ = llava_pair(tmp_path)
    if lora:
        A.apply_lora(dict(PEFT))
        wake_adapters(A)
    A.eval()
    eng = A.engine
    assert A.is_packed and eng.wide_gemv and eng.wide_gemv_w4
    rep = ROWS // batch["prompt_input_ids"].shape[0]
    kw = dict(input_ids=batch["prompt_input_ids"].repeat(rep, 1).to(gpu), attention_mask=batch["prompt_attention_mask"].repeat(rep, 1).to(gpu),
              pixel_values=batch["img_input_dict"]["pixel_values"].repeat(rep, 1, 1, 1).to(gpu), max_new_tokens=NEW, do_sample=False,
              pad_token_id=0, eos_token_id=10 ** 6)
    assert kw["input_ids"].shape[0] == ROWS
    layer = "vlr_decoder_layer_decode_w4_lora" if lora else "vlr_decoder_layer_decode_w4"
    need16, need_wide = decoder_scratch_need(eng, lora)
    assert need16 < need_wide

    def run():
        s = Spy(A, monkeypatch)
        out = A.generate(**kw)
        scratch = [v["gemv"].numel() for k, v in eng._ws.items() if isinstance(k, tuple) and k and k[0] == "decode_ws"]
        monkeypatch.undo()
        assert s.calls == 1 and s.steps == NEW - 1 and s.names.count(layer) == (NEW - 1) * eng.L and len(s.logits) == NEW
        assert "vlr_gptq_dequant_bf16" not in s.names[s.names.index(layer):], "decoding streams the packed weights"
        assert len(scratch) == 1
        return out, s, scratch[0]

    wide, sw, bytes_wide = run()
    assert bytes_wide >= need_wide, "scratch that makes the packed layer take its 64-row groups"
    assert sw.names.count("vlr_gemv_wide_bf16") == NEW - 1 and "vlr_gemv_bf16" not in sw.names, "the lm-head: one wide call per step"
    eng.wide_gemv = False
    groups, sg, bytes_groups = run()
    assert need16 <= bytes_groups < need_wide, "scratch that keeps the packed layer on 16-row groups"
    assert sg.names.count("vlr_gemv_bf16") == 2 * (NEW - 1) and "vlr_gemv_wide_bf16" not in sg.names
    assert torch.equal(wide, groups)
    for k, (a, b) in enumerate(zip(sw.logits, sg.logits)):
        assert torch.isfinite(a[:ROWS]).all() and torch.equal(a[:ROWS], b[:ROWS]), f"logits of step {k}"
    assert torch.equal(wide[:2], wide[2:4]), "repeated rows decode alike"
    assert wide.shape == (ROWS, kw["input_ids"].shape[1] + NEW)
