"""Free-form answers to a question file (the reference's src/vlrlhf/eval/vqa/generate.py): --file_path is a JSON list of
{"image": path under --data_root, "prompt": question}; --output_path receives the rows with "response" added."""
import argparse
import json
import os

from ..utils import Shard, VLCollator, add_shard_args, finish, run_vqa


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--data_root", type=str)
    p.add_argument("--file_path", type=str)
    p.add_argument("--model_path", type=str, default="llava-hf/llava-1.5-7b-hf")
    p.add_argument("--processor_path", type=str, default=None)
    p.add_argument("--output_path", type=str, default="vqa_result.json")
    p.add_argument("--batch_size", type=int, default=16)
    return add_shard_args(p).parse_args(argv)


class VQADataset:
    def __init__(self, data_root, file_path):
        with open(file_path) as f:
            self.data = json.load(f)
        self.data_root = data_root

    def __len__(self):
        return len(self.data)

    def __getitem__(self, index):
        q = self.data[index]
        return dict(image=os.path.join(self.data_root, q["image"]), prompt=q["prompt"])


class Collator(VLCollator):
    def __call__(self, batch):
        images = [b["image"] for b in batch]
        prompts = [self.processor.format_multimodal_prompt(b["prompt"], b["image"]) for b in batch]
        inputs = self.processor(texts=prompts, images_path=images, padding_side="left", check_format=False)
        return inputs, [dict(image=b["image"], prompt=b["prompt"]) for b in batch]


def finalize(rows, output_path):
    with open(output_path, "w") as f:
        json.dump(rows, f, indent=4)
    return rows


def main(argv=None):
    args = parse_args(argv)
    dataset = Shard(VQADataset(args.data_root, args.file_path), args.num_shards, args.shard_id)
    rows = run_vqa(args.model_path, dataset, Collator, None, args.processor_path, args.batch_size)
    return finish("vqa.generate", rows, args)


if __name__ == "__main__":
    main()
