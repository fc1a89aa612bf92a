#!/usr/bin/env python3
"""Times the KTO loss kernel and one KTO step beside a DPO step over the same sequences, and appends the figures to profiles/kto.txt:
    python tools/kto_bench.py [--rows 8] [--text_len 512] [--steps 3] [--warmup 1] [--layers 32] [--skip_step] [--out profiles/kto.txt]
Kernel: vlr_kto_loss alone (8, 64 and 1024 main rows with as many KL rows), alternating launch by launch with a device-to-device copy
that moves the same HBM traffic - clocks and co-tenants drift over both alike - HIP events around every launch, medians reported.
Step: LLaVA-1.5-7B widths, LoRA r 64, random weights, `rows` main rows of text_len text tokens (half prompt, half completion): HIP
events around VLKTOTrainer.training_step (the adapter-off reference pass over [main ; KL], the no-grad policy pass over the KL rows, the
training pass over the main rows, the loss, the backward) and the optimizer step.  The yardstick, from the same process: a DPO step
over rows / 2 pairs - the same number of sequences of the same shape - timed the same way."""
import argparse
import gc
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vl-rlhf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ppo_bench import _alternate  # noqa: E402


def kernels(lines):
    from vlrlhf import _hip as hip
    g = torch.Generator(device="cuda").manual_seed(0)
    for n in (8, 64, 1024):
        ref, ref_kl = -200 * torch.rand(n, generator=g, device="cuda"), -200 * torch.rand(n, generator=g, device="cuda")
        pi, pi_kl = ref + torch.randn(n, generator=g, device="cuda") * 5, ref_kl + torch.randn(n, generator=g, device="cuda") * 5
        label = (torch.arange(n, device="cuda") % 2).to(torch.uint8)
        out = [torch.empty(n, device="cuda") for _ in range(3)]
        st = torch.empty(8, device="cuda")
        traffic = (4 * n + 3 * n) * 4 + n      # four inputs, three outputs, the labels
        k, c = _alternate(lambda: hip.call("vlr_kto_loss", pi, ref, label, n, pi_kl, ref_kl, n, 0.1, 1.0, 1.0, 1.0, *out, st), traffic)
        lines.append(f"vlr_kto_loss n={n:5d} m={n:5d}        {k * 1e3:9.1f} us   copy moving {traffic / 1e6:8.4f} MB {c * 1e3:9.1f} us")


def _steps(tr, model, batch, a):
    step_ms, opt_ms = [], []
    for k in range(a.warmup + a.steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        tr.training_step(model, batch)
        ev[1].record()
        model.engine.optimizer_step(lr=1e-6, beta1=0.9, beta2=0.98, eps=1e-6, weight_decay=0.0, max_grad_norm=1.0)
        ev[2].record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            step_ms.append(ev[0].elapsed_time(ev[1]))
            opt_ms.append(ev[1].elapsed_time(ev[2]))
    return step_ms, opt_ms


def _report(lines, rows):
    for name, v in rows:
        lines.append(f"{name:72s} median {statistics.median(v):9.2f} ms   min {min(v):9.2f}   max {max(v):9.2f}")


def step(a, lines):
    from vlrlhf.base.collator import VLDPODataCollatorWithPadding, VLKTODataCollatorWithPadding
    from vlrlhf.base.trainer import KTOConfig
    from vlrlhf.models.Llava import LlavaDPOTrainer, LlavaForRL, LlavaKTOTrainer
    from vlrlhf.utils.synthetic import LLAVA_1_5_7B, init_random_model, synthetic_batch
    cfg = dict(LLAVA_1_5_7B, layers=a.layers)
    lora = dict(r=64, lora_alpha=16, lora_dropout=0.0, target_modules="auto", bias="none", seed=0)
    B = a.rows

    def model_():
        m = LlavaForRL(cfg)
        del_ref = init_random_model(m, seed=0, std=0.02, policy_delta=1e-3)
        del del_ref
        return m

    # ---- KTO: B main rows, their B KL rows
    model = model_()
    tr = LlavaKTOTrainer(model, None, KTOConfig(per_device_train_batch_size=B), peft_config=lora)
    sb = synthetic_batch(B, a.text_len, cfg["image_token"], 32000, cfg["image_size"], seed=1234)
    rows = [{f"completion_{k}": sb[f"chosen_{k}"][i].tolist() for k in ("input_ids", "attention_mask", "labels")} | dict(label=i % 2 == 0, img_path=i)
            for i in range(B)]
    kb = VLKTODataCollatorWithPadding(VLDPODataCollatorWithPadding(0, -100), max_length=1 << 20, max_prompt_length=1 << 19)(rows)
    kb["img_input_dict"] = sb["img_input_dict"]
    kb = tr._prepare_inputs(kb)
    s_kto, o_kto = _steps(tr, model, kb, a)
    S = a.text_len + (cfg["image_size"] // cfg["patch_size"]) ** 2 - 1
    lines.append(f"KTO step: {B} main rows + {B} KL rows x {a.text_len} text tokens (S = {S}), {a.layers} layers, LLaVA-1.5-7B widths, LoRA r 64, "
                 f"{a.steps} timed after {a.warmup} warm-up")
    _report(lines, (("training_step (reference 2B rows, no-grad policy B KL rows, training pass B rows, loss, backward)", s_kto),
                    ("optimizer step", o_kto)))
    del tr, model
    gc.collect()
    torch.cuda.empty_cache()
    # ---- the yardstick: a DPO step over B / 2 pairs = the same B sequences in the training pass
    model = model_()
    args = SimpleNamespace(gradient_accumulation_steps=1, per_device_train_batch_size=B // 2)
    dtr = LlavaDPOTrainer(model, None, 0.1, 0, "sigmoid", args, None, -100, 0, "keep_end", None, None, None, peft_config=lora)
    db = dtr._prepare_inputs(synthetic_batch(B // 2, a.text_len, cfg["image_token"], 32000, cfg["image_size"], seed=1234))
    s_dpo, o_dpo = _steps(dtr, model, db, a)
    lines.append(f"DPO step, the yardstick: {B // 2} pairs = {B} sequences of the same shape")
    _report(lines, (("training_step (reference 2 x B/2 rows, training pass 2 x B/2 rows, loss, backward)", s_dpo), ("optimizer step", o_dpo)))
    lines.append(f"training_step medians: KTO {statistics.median(s_kto):.2f} ms, DPO {statistics.median(s_dpo):.2f} ms "
                 f"(KTO runs 2B reference rows and B more no-grad policy rows than the DPO step of B sequences; the backward is over B rows in both)")


def main():
    p = argparse.ArgumentParser()
    for k, v in dict(rows=8, text_len=512, steps=3, warmup=1, layers=32).items():
        p.add_argument(f"--{k}", type=int, default=v)
    p.add_argument("--skip_step", action="store_true")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "kto.txt"))
    a = p.parse_args()
    lines = [f"# tools/kto_bench.py {time.strftime('%Y-%m-%d')}, {torch.cuda.get_device_name(0)} (1 box, 1 run): the kernel alone, alternating with a device "
             "copy moving the same bytes (read + write) (medians of 30 launches, HIP events)"]
    kernels(lines)
    if not a.skip_step:
        step(a, lines)
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
