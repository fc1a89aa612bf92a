#!/usr/bin/env python3
"""Times one supervised fine-tuning step and the policy half of a DPO step of the same row count:
    python tools/sft_time.py [--rows 4] [--text_len 2048] [--lora_r 128] [--steps 8] [--warmup 3] [--layers 32]
LLaVA-1.5-7B shapes, random weights, LoRA, gradient checkpointing, four resident batches.  SFT: `rows` sequences, labels on the second
half of the text.  DPO policy half: rows/2 pairs (chosen + rejected = `rows` sequences of the same length) with the reference log-probs
stored on the batch (no reference pass).  Both steps = loss + backward + clip + AdamW; HIP events around each step, median reported."""
import argparse
import os
import statistics
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vl-rlhf_amd"))


def timed(step, n, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        step()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms), min(ms), max(ms)


def main():
    p = argparse.ArgumentParser()
    for k, v in dict(rows=4, text_len=2048, lora_r=128, steps=8, warmup=3, layers=32).items():
        p.add_argument(f"--{k}", type=int, default=v)
    a = p.parse_args()
    from vlrlhf.models.Llava import LlavaDPOTrainer, LlavaForRL, LlavaSFTTRainer
    from vlrlhf.utils.synthetic import LLAVA_1_5_7B, init_random_model, synthetic_batch
    cfg = dict(LLAVA_1_5_7B, layers=a.layers)
    hp = dict(lr=2e-5, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_grad_norm=1.0)
    peft = dict(r=a.lora_r, lora_alpha=2 * a.lora_r, lora_dropout=0.0, target_modules="auto", bias="none", seed=0)
    out = {}
    for mode in ("sft", "dpo_policy_half"):
        model = LlavaForRL(cfg)
        ref = init_random_model(model, seed=0, std=0.02, policy_delta=1e-3)
        del ref
        eng = model.engine
        eng.gradient_checkpointing = True
        args = SimpleNamespace(gradient_accumulation_steps=1)
        if mode == "sft":
            tr = LlavaSFTTRainer(model=model, args=args, peft_config=peft)
        else:
            tr = LlavaDPOTrainer(model, None, 0.1, 0, "sigmoid", args, None, -100, 0, peft_config=peft)
        gen = torch.Generator(device=eng.dev)
        gen.manual_seed(4321)
        for k, t_ in eng.lv.items():             # peft initialises B = 0: random B so that the adapter GEMMs do real arithmetic
            if ".b_" in k:
                t_.normal_(0.0, 1e-3, generator=gen)
        eng.init_optimizer()
        batches = []
        for i in range(4):
            if mode == "sft":
                b = synthetic_batch(a.rows, a.text_len, cfg["image_token"], 32000, cfg["image_size"], seed=1234 + 1000 * i)
                b = dict(input_ids=b["chosen_input_ids"], attention_mask=b["chosen_attention_mask"], labels=b["chosen_labels"],
                         pixel_values=b["img_input_dict"]["pixel_values"])
            else:
                b = synthetic_batch(a.rows // 2, a.text_len, cfg["image_token"], 32000, cfg["image_size"], seed=1234 + 1000 * i)
                n = a.rows // 2
                b["reference_chosen_logps"], b["reference_rejected_logps"] = torch.full((n,), -9000.0), torch.full((n,), -9000.0)
            batches.append(tr._prepare_inputs(b))
        k = [0]

        def step():
            eng.zero_grad()
            tr.training_step(model, batches[k[0] % 4])
            eng.optimizer_step(**hp)
            k[0] += 1
        out[mode] = timed(step, a.steps, a.warmup)
        print(f"{mode:16s} {a.rows} x {a.text_len} tokens, LoRA r {a.lora_r}, checkpointing, {a.layers} layers: "
              f"median {out[mode][0]:.1f} ms (min {out[mode][1]:.1f}, max {out[mode][2]:.1f}) over {a.steps} steps", flush=True)
        del model, tr, eng, batches
        torch.cuda.empty_cache()
    print(f"ratio sft / dpo_policy_half = {out['sft'][0] / out['dpo_policy_half'][0]:.3f}")


if __name__ == "__main__":
    main()
