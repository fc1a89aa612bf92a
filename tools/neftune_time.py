#!/usr/bin/env python3
"""What NEFTune (neftune_noise_alpha) costs on the MI355X:
    python tools/neftune_time.py [--rows 8] [--text_len 1024] [--reps 30] [--steps 6] [--warmup 2] [--layers 32] [--lora_r 128]
                                 [--skip_steps] [--out profiles/neftune.txt]
1. vlr_neftune_add alone at the headline shape - `rows` sequences of `text_len` tokens with one image each (LLaVA-1.5: 576 image rows, so
   8 x 1599 merged rows at the defaults), H = 4096, on the bf16 and on the fp32 residual stream - next to a plain device copy of the same
   bytes (the text rows read once and written once), alternating in one process; HIP events around 20 back-to-back launches, median.
2. one SFT step and one DPO step (LLaVA-1.5-7B shapes, random weights, LoRA, gradient checkpointing, four resident batches; the DPO
   reference is the adapter-off pass of the same step) with alpha = 5 against alpha None on the SAME model, alternating blocks of
   `steps` steps; step = loss + backward + clip + AdamW, HIP events per step, median / min / max per block.  The noise is switched
   with engine.set_neftune directly (key = seed 42, rank 0), not through the trainer's _before_train / train(): the passes launch the
   same kernel either way.  `--layers 2 --steps 2` is the quick rehearsal of this half."""
import argparse
import os
import statistics
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vl-rlhf_amd"))

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def event_ms(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner


def kernel_alone(a):
    from vlrlhf import _hip
    from vlrlhf.engine import neftune_scale
    H, P, Bn, T = 4096, 576, a.rows, a.text_len
    S = T - 1 + P
    row = torch.cat([torch.tensor([0]), -(torch.arange(P) + 1), torch.arange(2, T)]).to(torch.int32)       # token 1 is the image
    src = torch.stack([torch.where(row < 0, row - b * P, row) for b in range(Bn)]).contiguous().cuda()
    n_text = int((src >= 0).sum())
    scale = neftune_scale(5.0, T, H)[1]
    say(f"kernel alone: {Bn} x {S} merged rows ({n_text} text rows noised, {Bn * P} image rows skipped), H = {H}, alpha 5 -> scale {scale:.3e}")
    for name, dt in (("bf16 stream", torch.bfloat16), ("fp32 stream", torch.float32)):
        x = (torch.randn(Bn * S, H, device="cuda") * 0.02).to(dt)
        a_, b_ = torch.empty(n_text, H, dtype=dt, device="cuda").normal_(), torch.empty(n_text, H, dtype=dt, device="cuda")
        call = [0]

        def noise():
            call[0] += 1
            _hip.call("vlr_neftune_add", x, int(dt == torch.float32), src, Bn, T, S, H, scale, 42, call[0], 0)

        def copy():
            b_.copy_(a_)
        for f in (noise, copy):
            event_ms(f, 20)
        tn, tc = [], []
        for _ in range(a.reps):                  # alternating: both see the same clocks and the same neighbours
            tn.append(event_ms(noise, 20))
            tc.append(event_ms(copy, 20))
        nbytes = 2 * n_text * H * x.element_size()
        for what, t in (("vlr_neftune_add", tn), ("copy of the same bytes", tc)):
            med = statistics.median(t)
            say(f"  {name}  {what:24s} median {med * 1e3:8.1f} us  (min {min(t) * 1e3:.1f}, max {max(t) * 1e3:.1f})  "
                f"{nbytes / 1e9:.3f} GB moved -> {nbytes / med / 1e9:.2f} TB/s")
        say(f"  {name}  ratio noise / copy = {statistics.median(tn) / statistics.median(tc):.2f}")


def steps(a):
    from vlrlhf.models.Llava import LlavaDPOTrainer, LlavaForRL, LlavaSFTTRainer
    from vlrlhf.utils.synthetic import LLAVA_1_5_7B, init_random_model, synthetic_batch
    cfg = dict(LLAVA_1_5_7B, layers=a.layers)
    hp = dict(lr=2e-5, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_grad_norm=1.0)
    peft = dict(r=a.lora_r, lora_alpha=2 * a.lora_r, lora_dropout=0.0, target_modules="auto", bias="none", seed=0)
    for mode in ("sft", "dpo"):
        model = LlavaForRL(cfg)
        ref = init_random_model(model, seed=0, std=0.02, policy_delta=1e-3)
        del ref
        eng = model.engine
        eng.gradient_checkpointing = True
        args = SimpleNamespace(gradient_accumulation_steps=1, seed=42)
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
            batches.append(tr._prepare_inputs(b))
        k = [0]

        def step():
            eng.zero_grad()
            tr.training_step(model, batches[k[0] % 4])
            eng.optimizer_step(**hp)
            k[0] += 1
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        say(f"{mode} step: {a.rows} sequences x {a.text_len} tokens + 1 image, LoRA r {a.lora_r}, checkpointing, {a.layers} layers")
        med = {None: [], 5.0: []}
        for block in range(4):                   # None, 5, None, 5 on the same model
            alpha = (None, 5.0)[block % 2]
            eng.set_neftune(alpha, seed=42, rank=0)
            before = eng._neftune_calls
            step()                               # (one unmeasured step after the switch)
            ms = [event_ms(step, 1) for _ in range(a.steps)]
            med[alpha].append(statistics.median(ms))
            say(f"  alpha {str(alpha):5s} median {med[alpha][-1]:8.2f} ms  (min {min(ms):.2f}, max {max(ms):.2f}) over {a.steps} steps, "
                f"{eng._neftune_calls - before} noise launches")
        eng.set_neftune(None)
        off, on = statistics.mean(med[None]), statistics.mean(med[5.0])
        spread = max(abs(med[None][0] - med[None][1]), abs(med[5.0][0] - med[5.0][1]))
        say(f"  alpha 5 - alpha None = {on - off:+.2f} ms ({(on - off) / off * 100:+.3f} %); block-to-block spread of one setting {spread:.2f} ms")
        del model, tr, eng, batches
        torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    for k, v in dict(rows=8, text_len=1024, reps=30, steps=6, warmup=2, layers=32, lora_r=128).items():
        p.add_argument(f"--{k}", type=int, default=v)
    p.add_argument("--skip_steps", action="store_true")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "neftune.txt"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("neftune_time.py measures on the MI355X: no GPU here, nothing measured")
    say(f"# tools/neftune_time.py --rows {a.rows} --text_len {a.text_len} --reps {a.reps} --steps {a.steps} --layers {a.layers} --lora_r {a.lora_r}"
        f"  ({torch.cuda.get_device_name(0)})")
    kernel_alone(a)
    if not a.skip_steps:
        steps(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
