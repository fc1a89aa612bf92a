"""CPU-only checks of the supervised fine-tuning surface: the collators against hand-written expectations, VLSFTTrainer.tokenize_row
against rows the reference's own tokenize_row produced (tests/golden/sft_tokenize.json, written by tests/golden/make_sft_golden.py), the
sft.py argument parsing, the registry slots and the C-ABI exports."""
import copy
import inspect
import json
import os
from types import SimpleNamespace

import pytest
import torch

from tests.golden_util import GOLDEN, TINY_PROCESSOR


def test_sft_collator_pads_right_and_rejects_unknown_keys():
    from vlrlhf.base.collator import VLSFTDataCollatorWithPadding
    col = VLSFTDataCollatorWithPadding(pad_token_id=7, label_pad_token_id=-100)
    feats = [dict(input_ids=[1, 2, 3], labels=[-100, 2, 3], attention_mask=[1, 0, 1], img_path="a.jpg"),
             dict(input_ids=[4], labels=[4], attention_mask=[1], img_path="b.jpg")]
    out = col(feats)
    assert out["input_ids"].tolist() == [[1, 2, 3], [4, 7, 7]] and out["input_ids"].dtype == torch.long
    assert out["labels"].tolist() == [[-100, 2, 3], [4, -100, -100]]
    assert out["attention_mask"].tolist() == [[1, 0, 1], [1, 0, 0]]
    assert out["img_path"] == ["a.jpg", "b.jpg"] and set(out) == {"input_ids", "labels", "attention_mask", "img_path"}
    with pytest.raises(ValueError, match="Unexpected key in batch 'token_type_ids'"):
        col([dict(input_ids=[1], token_type_ids=[0])])


def test_model_sft_collators_put_pixels_at_the_top_level():
    from vlrlhf.models.InternLMXC2 import InternLMXC2SFTDataCollatorWithPadding
    from vlrlhf.models.Llava import LlavaSFTDataCollatorWithPadding
    from vlrlhf.models.LlavaNext import LlavaNextSFTDataCollatorWithPadding
    from vlrlhf.models.QwenVL import QwenVLSFTDataCollatorWithPadding
    row = lambda img: dict(input_ids=[1, 2], labels=[-100, 2], attention_mask=[1, 1], img_path=img)      # noqa: E731
    px = [torch.full((3, 4, 4), float(i)) for i in range(2)]
    out = LlavaSFTDataCollatorWithPadding(0, -100)([row(px[0]), row(px[1])])
    assert set(out) == {"input_ids", "labels", "attention_mask", "pixel_values"}          # img_path dropped, as the reference does
    assert tuple(out["pixel_values"].shape) == (2, 3, 4, 4) and float(out["pixel_values"][1].mean()) == 1.0
    tiles = [dict(pixel_values=torch.ones(2, 3, 4, 4), image_size=(8, 4)), dict(pixel_values=torch.ones(3, 3, 4, 4), image_size=(4, 8))]
    out = LlavaNextSFTDataCollatorWithPadding(0, -100)([row(tiles[0]), row(tiles[1])])
    assert set(out) == {"input_ids", "labels", "attention_mask", "pixel_values", "image_sizes"}
    assert tuple(out["pixel_values"].shape) == (2, 3, 3, 4, 4) and out["image_sizes"].tolist() == [[8, 4], [4, 8]]
    out = QwenVLSFTDataCollatorWithPadding(0, -100)([row("a.jpg"), row("b.jpg")])
    assert set(out) == {"input_ids", "labels", "attention_mask"}                          # Qwen-VL reads its images from the ids
    proc = SimpleNamespace(image_processor=lambda items: torch.stack(list(items)))
    out = InternLMXC2SFTDataCollatorWithPadding(0, -100, proc)([row(px[0]), row(px[1])])
    assert set(out) == {"input_ids", "labels", "attention_mask", "pixel_values"} and tuple(out["pixel_values"].shape) == (2, 3, 4, 4)


def _sft_trainer(max_seq_length, **kw):
    from vlrlhf.models.Llava import LlavaProcessor, LlavaSFTTRainer
    proc = LlavaProcessor(TINY_PROCESSOR)
    proc.train()
    model = SimpleNamespace(engine=None)
    return LlavaSFTTRainer(model=model, args=SimpleNamespace(), processor=proc, max_seq_length=max_seq_length, **kw)


def test_tokenize_row_matches_the_reference_bit_for_bit():
    cases = json.load(open(os.path.join(GOLDEN, "sft_tokenize.json")))
    assert {c["name"] for c in cases} == {"multi_turn", "single_turn", "truncated"}
    for c in cases:
        tr = _sft_trainer(c["max_seq_length"])
        row = tr.tokenize_row(dict(conversations=copy.deepcopy(c["conversations"]), img_path=c["img_path"]))
        for k in ("input_ids", "attention_mask", "labels"):
            assert list(row[k]) == c[k], (c["name"], k)
        assert row["img_path"] == c["img_path"] and set(row) == {"input_ids", "attention_mask", "labels", "img_path"}
    multi = next(c for c in cases if c["name"] == "multi_turn")
    eos = multi["eos_token_id"]
    inside = [i for i, t in enumerate(multi["input_ids"][:-1]) if t == eos]
    assert len(inside) == 2, "the multi-turn fixture must hold eos tokens inside the conversation"
    assert all(multi["attention_mask"][i] == 0 and multi["labels"][i] == -100 for i in inside)          # the holes
    assert multi["input_ids"][-1] == eos and multi["attention_mask"][-1] == 1 and multi["labels"][-1] == eos
    trunc = next(c for c in cases if c["name"] == "truncated")
    assert len(trunc["input_ids"]) == trunc["max_seq_length"]


def test_sft_trainer_prepares_datasets_and_refuses_neftune():
    from vlrlhf.utils.data import DATASET_MAP
    rows = DATASET_MAP["synthetic_conversations"](SimpleNamespace(synthetic_rows=6, synthetic_image_size=28))
    assert all(len(r["conversations"]) >= 4 for r in rows) and any(len(r["conversations"]) == 6 for r in rows)      # multi-turn
    tr = _sft_trainer(64, train_dataset=rows, packing=True, dataset_text_field="text")          # packing accepted and ignored
    eos = tr.tokenizer.eos_token_id
    for r, raw in zip(tr.train_dataset, rows):
        assert set(r) == {"input_ids", "labels", "attention_mask", "img_path"} and len(r["input_ids"]) <= 64
        assert 0 in r["attention_mask"][:-1], "every synthetic conversation exercises the eos-hole path"
        assert all((m == 0) == (t == eos) for t, m in zip(r["input_ids"][:-1], r["attention_mask"][:-1]))
        assert not raw["conversations"][0]["value"].startswith("<image>")          # the caller's rows are not edited in place
    with pytest.raises(NotImplementedError, match="neftune"):
        _sft_trainer(64, neftune_noise_alpha=5.0)
    from vlrlhf.base.trainer import VLDPOTrainer, VLSFTTrainer, VLTrainerLoop
    assert issubclass(VLSFTTrainer, VLTrainerLoop) and issubclass(VLDPOTrainer, VLTrainerLoop)
    assert VLSFTTrainer.train is VLDPOTrainer.train and VLSFTTrainer.evaluate is VLDPOTrainer.evaluate          # one loop, not a copy
    # the reference's constructor signature, in order (base/trainer.py:574-601)
    names = list(inspect.signature(VLSFTTrainer.__init__).parameters)[1:]
    assert names == ["model", "args", "data_collator", "train_dataset", "eval_dataset", "processor", "model_init", "compute_metrics",
                     "callbacks", "optimizers", "preprocess_logits_for_metrics", "peft_config", "dataset_text_field", "packing",
                     "formatting_func", "max_seq_length", "infinite", "num_of_sequences", "chars_per_token", "dataset_num_proc",
                     "dataset_batch_size", "neftune_noise_alpha", "model_init_kwargs", "dataset_kwargs", "eval_packing"]


def test_sft_argument_parsing():
    from vlrlhf import sft
    from vlrlhf.dpo import _parse
    s, t, l = _parse(sft.ScriptArguments, sft.TrainingArguments, sft.LoraArguments,
                     argv=["--dataset_name", "vlquery_json", "--data_path", "q.json", "--image_root", "/img", "--max_length", "2048",
                           "--merge_peft_model", "True", "--use_lora", "True", "--lora_r", "128", "--gradient_checkpointing", "True",
                           "--per_device_train_batch_size", "4", "--learning_rate", "2e-5", "--eval_strategy", "steps"])
    assert (s.dataset_name, s.data_path, s.image_root, s.max_length, s.merge_peft_model) == ("vlquery_json", "q.json", "/img", 2048, True)
    assert s.freeze_vision_tower is True and s.label_pad_token_id == -100 and s.data_ratio == 1.0
    assert t.use_lora and t.gradient_checkpointing and t.per_device_train_batch_size == 4 and t.learning_rate == 2e-5
    assert t.evaluation_strategy == "steps" and l.lora_r == 128
    d = _parse(sft.ScriptArguments, sft.TrainingArguments, sft.LoraArguments, argv=[])
    assert d[0].dataset_name is None and d[0].merge_peft_model is False and d[1].learning_rate == 5e-5 and d[1].adam_beta2 == 0.999
    assert not hasattr(d[0], "beta") and not hasattr(d[0], "loss_type")


def test_vlquery_json_adds_img_path(tmp_path):
    from vlrlhf.utils.data import DATASET_MAP
    p = tmp_path / "q.json"
    conv = [{"from": "user", "value": "hi"}, {"from": "assistant", "value": "ho"}]
    p.write_text(json.dumps([dict(conversations=conv, image="x/1.jpg")]))
    rows = DATASET_MAP["vlquery_json"](SimpleNamespace(data_path=str(p), image_root="/root_dir"))
    assert rows == [dict(conversations=conv, image="x/1.jpg", img_path="/root_dir/x/1.jpg")]


def test_registry_slots_and_auto_classes():
    from vlrlhf.base.collator import VLSFTDataCollatorWithPadding
    from vlrlhf.base.trainer import VLSFTTrainer
    from vlrlhf.utils import auto_load
    for arch in ("LlavaForConditionalGeneration", "LlavaNextForConditionalGeneration", "QWenLMHeadModel", "InternLMXComposer2ForCausalLM"):
        cm = auto_load.auto_core_mapper(arch)
        assert cm.sft_collator is not None and issubclass(cm.sft_collator, VLSFTDataCollatorWithPadding), arch
        assert cm.sft_trainer is not None and issubclass(cm.sft_trainer, VLSFTTrainer), arch
    assert hasattr(auto_load, "MyAutoSFTCollator") and hasattr(auto_load, "MyAutoSFTTrainer")


def test_sft_exports_are_in_the_library():
    from vlrlhf import _hip
    l = _hip.lib()
    for name in ("vlr_ce_mean_fwd", "vlr_ce_mean_workspace_bytes", "vlr_lmhead_ce_bwd", "vlr_lmhead_ce_row_block"):
        assert hasattr(l, name) and name in _hip.exported_symbols(), name
    assert _hip.helper("vlr_ce_mean_workspace_bytes") >= 4
    # argument errors surface without a GPU
    assert l.vlr_ce_mean_fwd(None, 4, None, None, None) == 1 and b"vlr_ce_mean_fwd" in l.vlr_last_error()
    assert l.vlr_lmhead_ce_bwd(None, None, None, None, None, None, None, None, None, None, 0, 8, 8, 8, 0, None) == 1
    # the default block is a multiple of the GEMM's 256-row tile and keeps d logits (+ fp32 logits) of a block under 1 GiB
    for V in (32000, 151936):
        rb = _hip.helper("vlr_lmhead_ce_row_block", 65536, V, 4096)
        assert rb % 256 == 0 and 256 <= rb < 65536 and rb * V * 6 + int(l.vlr_lmhead_workspace_bytes(rb, V)) <= 1 << 30, (V, rb)
    assert _hip.helper("vlr_lmhead_ce_row_block", 100, 32000, 4096) == 100
