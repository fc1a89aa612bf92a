#!/usr/bin/env python3
"""Writes tests/golden/sft_tokenize.json: ids, attention masks and labels produced by the REFERENCE's own
VLSFTTrainer.tokenize_row (src/vlrlhf/base/trainer.py:631-654) and LlavaProcessor.process_batch_conv on the committed
tests/golden/tiny_llava_processor, for a multi-turn conversation (eos tokens inside: the masked holes), a single-turn one and a
truncated one.  Data fixture for tests/test_sft_host.py.  Runs only where the reference is mounted; trl / peft / deepspeed are
absent there, so the reference is imported under the stubs of the oracle/ generators."""
import copy
import importlib.machinery
import json
import os
import sys
import types

import transformers
from transformers import PreTrainedModel, AutoModelForCausalLM, Trainer, TrainingArguments, PreTrainedTokenizerBase  # noqa: F401  (before the stubs)
from transformers.trainer_callback import TrainerCallback  # noqa: F401
from transformers.trainer_utils import EvalPrediction, EvalLoopOutput  # noqa: F401
from transformers.tokenization_utils_base import BatchEncoding  # noqa: F401
import accelerate.utils  # noqa: F401
import datasets  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = "/root/reference/src"
CASES = [
    dict(name="multi_turn", max_seq_length=512, img_path="a.jpg", conversations=[
        {"from": "user", "value": "What is shown in this picture?"},
        {"from": "assistant", "value": "A small brown dog is running across the green field.</s>"},
        {"from": "user", "value": "What colour is the car?"},
        {"from": "assistant", "value": "The car is red and it is parked near the house.</s>"},
        {"from": "user", "value": "Is there a cat in the photo?"},
        {"from": "assistant", "value": "No, there is no cat, but there is a bird on the fence."}]),
    dict(name="single_turn", max_seq_length=512, img_path="b.jpg", conversations=[
        {"from": "user", "value": "<image>How many apples are on the table?"},
        {"from": "assistant", "value": "There are three apples and one orange on the table."}]),
    dict(name="truncated", max_seq_length=24, img_path="c.jpg", conversations=[
        {"from": "user", "value": "Describe the image in detail."},
        {"from": "assistant", "value": "The image shows two people sitting at a wooden table with cups of coffee.</s>"},
        {"from": "user", "value": "And then?"},
        {"from": "assistant", "value": "the quick brown fox jumps over the lazy dog"}]),
]


def _install_stubs():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__spec__ = importlib.machinery.ModuleSpec(name, None)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class _Base:
        def __init__(self, *a, **k):
            pass

    class _Logger:
        def __getattr__(self, n):
            return lambda *a, **k: None

    mod("loguru", logger=_Logger())
    mod("wandb", Image=_Base)
    mod("trl", DPOTrainer=_Base, PPOTrainer=_Base, PPOConfig=_Base, SFTTrainer=_Base, RewardTrainer=_Base, RewardConfig=_Base,
        AutoModelForCausalLMWithValueHead=_Base)
    mod("trl.trainer")
    mod("trl.trainer.reward_config", RewardConfig=_Base)
    mod("peft", PeftConfig=_Base, LoraConfig=_Base, PeftModel=_Base, prepare_model_for_kbit_training=lambda *a, **k: None,
        get_peft_model=lambda *a, **k: None)
    mod("deepspeed", zero=types.SimpleNamespace(GatheredParameters=None))
    mod("deepspeed.runtime")
    mod("deepspeed.runtime.zero")
    mod("deepspeed.runtime.zero.partition_parameters", ZeroParamStatus=types.SimpleNamespace(NOT_AVAILABLE=0))
    ds = mod("transformers.deepspeed", is_deepspeed_zero3_enabled=lambda: False)
    transformers.__dict__["deepspeed"] = ds


def main():
    _install_stubs()
    sys.path.insert(0, REF_SRC)
    from vlrlhf.base.trainer import VLSFTTrainer
    from vlrlhf.models.Llava import LlavaProcessor
    proc = LlavaProcessor(os.path.join(HERE, "tiny_llava_processor"))
    proc.train()
    out = []
    for case in CASES:
        tr = object.__new__(VLSFTTrainer)          # tokenize_row reads these three attributes only
        tr.processor, tr.tokenizer, tr.max_seq_length = proc, proc.tokenizer, case["max_seq_length"]
        row = tr.tokenize_row(dict(conversations=copy.deepcopy(case["conversations"]), img_path=case["img_path"]))
        eos = proc.tokenizer.eos_token_id
        out.append(dict(case, eos_token_id=eos, input_ids=list(row["input_ids"]), attention_mask=list(row["attention_mask"]),
                        labels=list(row["labels"])))
        print(case["name"], len(row["input_ids"]), "eos inside:", sum(1 for t in row["input_ids"][:-1] if t == eos),
              "mask zeros:", row["attention_mask"].count(0))
    with open(os.path.join(HERE, "sft_tokenize.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
