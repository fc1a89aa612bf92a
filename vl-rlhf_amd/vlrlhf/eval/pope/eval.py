"""POPE: yes / no object-hallucination probes (the reference's src/vlrlhf/eval/pope/eval.py without its MySQL reporter).

--file_root is walked for question files (JSONL rows `image`, `text`, `label`); a file name says which split it is (random, popular,
adversarial).  Every question is answered greedily (utils.run_vqa) and the answers are scored per file.  --output_path receives
{"results": rows with response / label / category, "metrics": {file name: {acc, precision, recall, f1, yes_rate}}}."""
import argparse
import json
import os

from ..utils import Shard, VLCollator, add_shard_args, finish, run_vqa

SPLITS = (("popular", "popular"), ("adversarial", "adv"), ("random", "random"))      # tested in this order, as the reference does
NEGATIVE_WORDS = frozenset(("No", "not", "no"))


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--image_root", type=str)
    p.add_argument("--file_root", type=str)
    p.add_argument("--model_path", type=str, default="llava-hf/llava-1.5-7b-hf")
    p.add_argument("--processor_path", type=str, default=None)
    p.add_argument("--output_path", type=str, default="pope_result.json")
    p.add_argument("--batch_size", type=int, default=16)
    return add_shard_args(p).parse_args(argv)


def split_prefix(file_name):
    low = file_name.lower()
    for word, prefix in SPLITS:
        if word in low:
            return prefix
    raise ValueError(f"Unsupported file: {file_name}")


def normalise_answer(text):
    """a free-form answer -> "yes" / "no": the first sentence only, commas dropped, "no" when `No`, `no` or `not` is one of its
    space-separated words ("Nothing" is not), "yes" otherwise - the empty answer included"""
    first = text.split(".")[0]
    words = first.replace(",", "").split(" ")
    return "no" if NEGATIVE_WORDS.intersection(words) else "yes"


def evaluate(outputs):
    """rows with `response` and `label` -> the five POPE figures in percent, rounded to 2 places.  "yes" is the positive class; a label
    other than "no" counts as "yes".  Where the reference divides by zero and raises (no positive prediction, no positive label, or no
    true positive) the undefined ratio is reported as 0.0, so that a finished run still writes its answers."""
    pred = [normalise_answer(o["response"]) == "yes" for o in outputs]
    gold = [o["label"] != "no" for o in outputs]
    tp = sum(p and g for p, g in zip(pred, gold))
    fp = sum(p and not g for p, g in zip(pred, gold))
    tn = sum(not p and not g for p, g in zip(pred, gold))
    fn = sum(not p and g for p, g in zip(pred, gold))
    print(f"TP {tp}  FP {fp}  TN {tn}  FN {fn}")
    ratio = lambda a, b: a / b if b else 0.0      # noqa: E731
    precision, recall = ratio(tp, tp + fp), ratio(tp, tp + fn)
    figures = dict(acc=(tp + tn) / len(pred), precision=precision, recall=recall, f1=ratio(2 * precision * recall, precision + recall),
                   yes_rate=sum(pred) / len(pred))
    return {k: round(v * 100, 2) for k, v in figures.items()}


class CaptioningDataset:
    def __init__(self, image_root, file_path):
        with open(file_path) as f:
            self.data = [json.loads(line) for line in f if line.strip()]
        self.image_root = image_root

    def __len__(self):
        return len(self.data)

    def __getitem__(self, index):
        q = self.data[index]
        return dict(image=os.path.join(self.image_root, q["image"]), prompt=q["text"], label=q["label"])


class Collator(VLCollator):
    """left-padded prompts, the image placeholder put in by the family's processor"""

    def __call__(self, batch):
        images = [b["image"] for b in batch]
        prompts = [self.processor.format_multimodal_prompt(b["prompt"], b["image"]) for b in batch]
        inputs = self.processor(texts=prompts, images_path=images, padding_side="left", check_format=False)
        return inputs, [dict(label=b["label"]) for b in batch]


def question_files(file_root):
    """(path, file name) of every file under file_root, in os.walk order; an unknown name raises before any model is loaded"""
    found = [(os.path.join(root, fn), fn) for root, _, files in os.walk(file_root) for fn in sorted(files)]
    for _, fn in found:
        split_prefix(fn)
    return found


def finalize(rows, output_path):
    """rows of all files (each with `category` = its file name) -> metrics per file, everything written to output_path"""
    by_file = {}
    for r in rows:
        by_file.setdefault(r["category"], []).append(r)
    metrics = {}
    for fn, part in by_file.items():
        print(f"Results on {fn}")
        metrics[fn] = evaluate(part)
        print(" ".join(f"{split_prefix(fn)}_{k}={v}" for k, v in metrics[fn].items()))
    ordered = [r for part in by_file.values() for r in part]
    with open(output_path, "w") as f:
        json.dump(dict(results=ordered, metrics=metrics), f, indent=4)
    return metrics


def main(argv=None):
    args = parse_args(argv)
    rows = []
    for path, fn in question_files(args.file_root):
        dataset = Shard(CaptioningDataset(args.image_root, path), args.num_shards, args.shard_id)
        for r in run_vqa(args.model_path, dataset, Collator, None, args.processor_path, args.batch_size):
            r["category"] = fn
            rows.append(r)
    return finish("pope.eval", rows, args)


if __name__ == "__main__":
    main()
