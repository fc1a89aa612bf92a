#!/usr/bin/env python3
"""Times one reward-model step against the --precomputed_ref DPO step of the SAME process, alternating:
    python tools/rm_bench.py [--pairs 4] [--text_len 1024] [--steps 6] [--warmup 2] [--layers 32] [--out profiles/reward_model.txt]
LLaVA-1.5-7B shapes of the default benchmark (bench.py: full fine-tune, 4 pairs, 1024 text tokens -> S = 1599, four resident batches),
random weights, ONE model carrying the reward head: the DPO trainer drives its base wrapper with the reference log-probs stored on the
batch (no reference pass), the RM trainer the reward model.  Both steps = loss + backward + clip + AdamW over the same flat buffers, so
the DPO step is the RM step's decoder work plus the lm-head (forward, d logits, dgrad, wgrad).  The two alternate step by step - clocks,
allocator state and co-tenants drift over both alike; HIP events around each step, medians reported and appended to --out."""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vl-rlhf_amd"))


def main():
    p = argparse.ArgumentParser()
    for k, v in dict(pairs=4, text_len=1024, steps=6, warmup=2, layers=32).items():
        p.add_argument(f"--{k}", type=int, default=v)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "reward_model.txt"))
    a = p.parse_args()
    from vlrlhf.models.Llava import LlavaDPOTrainer, LlavaForRM, LlavaRewardModel, LlavaRMTrainer
    from vlrlhf.utils.synthetic import LLAVA_1_5_7B, init_random_model, synthetic_batch
    cfg = dict(LLAVA_1_5_7B, layers=a.layers)
    hp = dict(lr=2e-8, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_grad_norm=1.0)
    base = LlavaForRM(cfg)
    ref = init_random_model(base, seed=0, std=0.02, policy_delta=1e-3)
    del ref
    model = LlavaRewardModel(base, seed=0)
    eng = model.engine
    args = SimpleNamespace(gradient_accumulation_steps=1)
    dpo = LlavaDPOTrainer(base, None, 0.1, 0, "sigmoid", args, None, -100, 0, precompute_ref_log_probs=True)
    rm = LlavaRMTrainer(model, args)
    eng.init_optimizer()
    d_batches, r_batches = [], []
    for i in range(4):
        b = synthetic_batch(a.pairs, a.text_len, cfg["image_token"], 32000, cfg["image_size"], seed=1234 + 1000 * i)
        r_batches.append(rm._prepare_inputs(dict(
            input_ids_chosen=b["chosen_input_ids"], attention_mask_chosen=b["chosen_attention_mask"],
            input_ids_rejected=b["rejected_input_ids"], attention_mask_rejected=b["rejected_attention_mask"],
            img_input_dict=dict(b["img_input_dict"]))))
        b["reference_chosen_logps"], b["reference_rejected_logps"] = torch.full((a.pairs,), -9000.0), torch.full((a.pairs,), -9000.0)
        d_batches.append(dpo._prepare_inputs(b))

    def step(tr, m, batch):
        eng.zero_grad()
        tr.training_step(m, batch)
        eng.optimizer_step(**hp)

    ms = {"rm": [], "dpo_precomputed_ref": []}
    for k in range(a.warmup + a.steps):
        for name, tr, m, bs in (("rm", rm, model, r_batches), ("dpo_precomputed_ref", dpo, base, d_batches)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            step(tr, m, bs[k % 4])
            e.record()
            torch.cuda.synchronize()
            if k >= a.warmup:
                ms[name].append(s.elapsed_time(e))
    S = a.text_len + (cfg["image_size"] // cfg["patch_size"]) ** 2 - 1
    lines = [f"# tools/rm_bench.py {time.strftime('%Y-%m-%d')}: {a.pairs} pairs x {a.text_len} text tokens (S = {S}), {a.layers} layers, LLaVA-1.5-7B widths, "
             f"full fine-tune, alternating steps of one process, {a.steps} timed after {a.warmup} warm-up, {torch.cuda.get_device_name(0)}"]
    for name, v in ms.items():
        lines.append(f"{name:22s} median {statistics.median(v):9.2f} ms   min {min(v):9.2f}   max {max(v):9.2f}")
    lines.append(f"ratio rm / dpo_precomputed_ref = {statistics.median(ms['rm']) / statistics.median(ms['dpo_precomputed_ref']):.4f}")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
