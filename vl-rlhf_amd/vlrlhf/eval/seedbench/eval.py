"""SEED-Bench image questions answered by perplexity (the reference's src/vlrlhf/eval/seedbench/eval.py).

Every question with question_type_id <= 9 (the image tasks; 10+ are video) becomes four rows, one per option, whose assistant turn is
"The answer is: " + the option.  utils.run_vqa_ppl gives each row the mean negative log-likelihood of its answer tokens; the option with
the strictly smallest value is the model's answer - on a tie the option seen first stays.  --output_path receives
{question_id: {"choice": letter, "ppl": value}}, the file seedbench.calculate scores."""
import argparse
import json
import os

from ..utils import Shard, VLCollator, add_shard_args, finish, run_vqa_ppl

CHOICES = ("A", "B", "C", "D")
LAST_IMAGE_TYPE = 9
ANSWER_PREFIX = "The answer is: "


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--data_root", type=str, default=None)
    p.add_argument("--model_path", type=str, default="llava-hf/llava-1.5-7b-hf")
    p.add_argument("--output_path", type=str, default="seedbench_result.json")
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--processor_path", type=str, default=None)
    return add_shard_args(p).parse_args(argv)


def expand_questions(questions, data_root):
    """image questions -> one row per (question, option), options in A..D order, questions in file order"""
    rows = []
    for q in questions:
        if q["question_type_id"] > LAST_IMAGE_TYPE:
            continue
        image = os.path.join(data_root, "SEED-Bench-image", q["data_id"])
        for letter in CHOICES:
            rows.append(dict(question_id=q["question_id"], image=image, prompt=q["question"],
                             response=ANSWER_PREFIX + q["choice_" + letter.lower()], choice=letter))
    return rows


class SeedbenchDataset:
    def __init__(self, data_root):
        with open(os.path.join(data_root, "SEED-Bench.json")) as f:
            self.data = expand_questions(json.load(f)["questions"], data_root)

    def __len__(self):
        return len(self.data)

    def __getitem__(self, index):
        return self.data[index]


class Collator(VLCollator):
    """right-padded single-turn conversations: the labels cover the assistant's words"""

    def __call__(self, batch):
        images = [b["image"] for b in batch]
        fmt = self.processor.format_multimodal_prompt
        convs = [self.processor.make_single_turn_conv(fmt(b["prompt"], b["image"]), b["response"]) for b in batch]
        inputs = self.processor(convs=convs, images_path=images, padding_side="right")
        return inputs, [dict(question_id=b["question_id"], choice=b["choice"]) for b in batch]


def pick_answers(rows):
    """rows with question_id / choice / ppl -> {question_id: {"choice", "ppl"}} of the strictly smallest ppl; ties (and nan, which is
    smaller than nothing) keep the first row seen"""
    best = {}
    for r in rows:
        cur = best.get(r["question_id"])
        if cur is None or r["ppl"] < cur["ppl"]:
            best[r["question_id"]] = dict(choice=r["choice"], ppl=r["ppl"])
    return best


def finalize(rows, output_path):
    answers = pick_answers(rows)
    with open(output_path, "w") as f:
        json.dump(answers, f)
    return answers


def main(argv=None):
    args = parse_args(argv)
    dataset = Shard(SeedbenchDataset(args.data_root), args.num_shards, args.shard_id)
    rows = run_vqa_ppl(args.model_path, dataset, Collator, None, args.processor_path, args.batch_size)
    return finish("seedbench.eval", rows, args)


if __name__ == "__main__":
    main()
