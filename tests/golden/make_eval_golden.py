#!/usr/bin/env python3
"""Writes the fixtures of tests/test_eval_host.py from the REFERENCE's own evaluation code, run on the CPU:

  eval_pope_cases.json      inputs of pope/eval.py's `evaluate` and the metric dicts it returned
  eval_seedbench.json       a six-question SEED-Bench file, the rows the reference's SeedbenchDataset expands it to, a recorded answer
                            file and what seedbench/calculate.py's `run_inference` returned for it
  eval_collators.json       input_ids / attention_mask (/ labels) of the reference's POPE and SEED-Bench collators over the reference's
                            LlavaProcessor on tests/golden/tiny_llava_processor (through the base VLProcessor.__call__, so no image file
                            is opened: the method of processor_answers.json["call"])

Runs only where the reference is mounted; the stubs of the absent third-party modules are those of oracle/make_golden.py (SURVEY.md
Appendix C) plus accelerate.Accelerator and pymysql, which the evaluation modules import and these functions never touch.
Usage:  python tests/golden/make_eval_golden.py"""
import importlib.machinery
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import make_golden  # noqa: E402,F401  (installs the stubs and puts the reference on sys.path)
import accelerate  # noqa: E402


class _Accelerator:
    device, is_local_main_process = "cpu", True

    def __init__(self, *a, **k):
        pass


accelerate.Accelerator = _Accelerator
_pymysql = types.ModuleType("pymysql")
_pymysql.__spec__ = importlib.machinery.ModuleSpec("pymysql", None)
sys.modules["pymysql"] = _pymysql

from vlrlhf.base.processor import VLProcessor as RefVLProcessor  # noqa: E402
from vlrlhf.eval.pope import eval as ref_pope  # noqa: E402
from vlrlhf.eval.seedbench import calculate as ref_calc  # noqa: E402
from vlrlhf.eval.seedbench import eval as ref_seed  # noqa: E402
from vlrlhf.models.Llava import LlavaProcessor as RefLlavaProcessor  # noqa: E402

# every case keeps TP, FP and FN above zero (checked below): the reference divides by TP + FP and TP + FN
POPE_CASES = {
    "plain": [("Yes", "yes"), ("No", "no"), ("Yes", "no"), ("No", "yes")],
    "comma_and_not": [("no,", "no"), ("There is not a dog.", "yes"), ("Yes, there is a dog in the image.", "yes"), ("Yes", "no")],
    "is_not": [("The cat is not there", "no"), ("is not", "yes"), ("yes", "yes"), ("It is", "no")],
    "first_sentence_only": [("Yes, there is. No other animal is visible.", "yes"), ("Yes, there is. No other...", "no"),
                            ("No. Yes it is.", "yes"), ("no", "no")],
    "empty_and_nothing": [("", "yes"), ("Nothing", "no"), ("Nothing", "yes"), ("not", "yes"), ("No", "no"), ("", "no")],
    "mixed": [("No", "no"), ("no,", "no"), ("is not", "no"), ("Yes, there is. No other...", "yes"), ("", "no"), ("Nothing", "yes"),
              ("no, it isn't", "yes"), ("Not really", "no"), ("yes", "yes"), ("NO", "no")],
}

SEED_QUESTIONS = dict(
    question_type={"Scene Understanding": 1, "Instance Identity": 2, "Instance Attributes": 3, "Action Recognition": 10, "Procedure Understanding": 12},
    questions=[
        dict(question_id="101", question_type_id=1, data_id="a.jpg", question="What is shown?", choice_a="A dog", choice_b="A cat", choice_c="A car", choice_d="A tree", answer="A"),
        dict(question_id="102", question_type_id=10, data_id="v1.mp4", question="What happens?", choice_a="run", choice_b="jump", choice_c="sit", choice_d="fall", answer="B"),
        dict(question_id="103", question_type_id=2, data_id="b.jpg", question="Which object is red?", choice_a="The car", choice_b="The house", choice_c="The bird", choice_d="The fence", answer="C"),
        dict(question_id="104", question_type_id=3, data_id="c.jpg", question="What colour is the car?", choice_a="red", choice_b="green", choice_c="brown", choice_d="white", answer="A"),
        dict(question_id="105", question_type_id=12, data_id="v2.mp4", question="What comes next?", choice_a="one", choice_b="two", choice_c="three", choice_d="four", answer="D"),
        dict(question_id="106", question_type_id=1, data_id="d.jpg", question="How many apples are on the table?", choice_a="one", choice_b="two", choice_c="three", choice_d="four", answer="C"),
    ])
SEED_ANSWERS = {"101": dict(choice="A", ppl=1.5), "103": dict(choice="C", ppl=2.25), "104": dict(choice="A", ppl=0.75),
                "106": dict(choice="D", ppl=3.0), "102": dict(choice="B", ppl=1.0), "105": dict(choice="D", ppl=1.0)}
# (every type keeps one right answer: the reference's run_inference raises KeyError for a type without any)


def dump(name, obj):
    path = os.path.join(HERE, name)
    with open(path, "w") as f:
        json.dump(obj, f, indent=1)
    print(f"[eval golden] {path} ({os.path.getsize(path)} bytes)")


def gen_pope():
    cases = []
    for name, pairs in POPE_CASES.items():
        outputs = [dict(response=r, label=l) for r, l in pairs]
        expected = ref_pope.evaluate(json.loads(json.dumps(outputs)))            # (it rewrites its argument's labels: hand it a copy)
        assert 0 < expected["precision"] < 100 and 0 < expected["recall"] < 100, (name, expected)      # TP, FP, FN all non-zero
        cases.append(dict(name=name, outputs=outputs, expected=expected))
    dump("eval_pope_cases.json", dict(cases=cases))


def gen_seedbench():
    with tempfile.TemporaryDirectory() as root:
        with open(os.path.join(root, "SEED-Bench.json"), "w") as f:
            json.dump(SEED_QUESTIONS, f)
        rows = [dict(r, image=os.path.relpath(r["image"], root)) for r in ref_seed.SeedbenchDataset(root).data]
    out = dict(questions=SEED_QUESTIONS, rows=rows, answers=SEED_ANSWERS, calculate={})
    ref_calc.data_type_id2name = {v: k for k, v in SEED_QUESTIONS["question_type"].items()}      # a global its __main__ sets
    for task in ("image", "all", "3"):
        out["calculate"][task] = ref_calc.run_inference(SEED_ANSWERS, ref_calc.filter_questions(SEED_QUESTIONS["questions"], task))
    dump("eval_seedbench.json", out)


def gen_collators():
    class Proc(RefLlavaProcessor):
        def __call__(self, *a, **k):                # the base method: tokens and padding, no image file is opened
            return RefVLProcessor.__call__(self, *a, **k)

    proc = Proc(os.path.join(HERE, "tiny_llava_processor"))
    proc.infer()
    pope_rows = [dict(image="img/a.jpg", prompt="Is there a cat in the photo?", label="no"),
                 dict(image="img/b.jpg", prompt="Is there a small brown dog running across the green field in the image?", label="yes")]
    seed_rows = [dict(question_id="101", image="img/a.jpg", prompt="What is shown in this picture?", response="The answer is: A small brown dog", choice="A"),
                 dict(question_id="101", image="img/a.jpg", prompt="What is shown in this picture?", response="The answer is: Two people sitting at a wooden table", choice="B"),
                 dict(question_id="104", image="img/b.jpg", prompt="What colour is the car?", response="The answer is: red", choice="A")]
    out = dict(pad_token_id=proc.tokenizer.pad_token_id)
    for name, collator, rows in (("pope", ref_pope.Collator, pope_rows), ("seedbench", ref_seed.Collator, seed_rows)):
        inputs, others = collator(proc)(json.loads(json.dumps(rows)))
        out[name] = dict(rows=rows, others=others, **{k: inputs[k].tolist() for k in ("input_ids", "attention_mask", "labels")})
        assert len({sum(m) for m in out[name]["attention_mask"]}) > 1, "rows of different length, so that the padding side shows"
    dump("eval_collators.json", out)


if __name__ == "__main__":
    gen_pope()
    gen_seedbench()
    gen_collators()
