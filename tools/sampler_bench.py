#!/usr/bin/env python3
"""generate's per-token selection on the MI355X: the stock torch ops against the one vlr_sample_tokens launch (sampler="device"), measured,
and appended to profiles/device_sampler.txt:

    python tools/sampler_bench.py [--layers 32] [--prompts 4] [--generations 8] [--new 256] [--blocks 3] [--skip_generate] [--out FILE]

Selection alone: the torch selection of LlavaForRL.generate (sampling_filter + softmax + torch.multinomial + where + one compare per eos
id), vlr_sample_tokens on the same logits, and a device copy of the logits' bytes (the floor: one read and one write of the rows), the
three ALTERNATING launch by launch in one process - same clocks, same neighbours - HIP events around each, 5 warm-up rounds, medians and
the spread (min .. max) of 30.  Shapes: B 4 and 32; V 32000 (T 1, top_k 50, top_p 1) and V 151936 with (1, 50, 1) and with Qwen-VL-Chat's
(1, 0, 0.3); the device sampler again with repetition_penalty 1.1 over 1024 history ids (the torch path has no penalty).
ms per new token: generate(sampler="torch") against generate(sampler="device") at the generate configuration of profiles/grpo.txt
(LLaVA-1.5-7B widths, random weights, LoRA r 64 live, `prompts` x `generations` rows over the shared prompt cache, `new` tokens, no row
ends early), `blocks` blocks of one call each, alternating; every block and the spread are reported."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vl-rlhf_amd"))

WARM, REPS = 5, 30


def _ev():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _fmt(v):
    return f"median {statistics.median(v) * 1e3:8.1f} us (min {min(v) * 1e3:8.1f}, max {max(v) * 1e3:8.1f})"


def selection(lines):
    from vlrlhf import _hip as hip
    from vlrlhf.models.Llava import sampling_filter
    gen = torch.Generator(device="cuda").manual_seed(0)
    eos = [2]
    for V, (T, k, p) in ((32000, (1.0, 50, 1.0)), (151936, (1.0, 50, 1.0)), (151936, (1.0, 0, 0.3))):
        for B in (4, 32):
            logits = torch.randn(B, V, generator=gen, device="cuda") * 3
            dst = torch.empty_like(logits)
            unf_t = torch.ones(B, dtype=torch.bool, device="cuda")
            unf = torch.ones(B, dtype=torch.uint8, device="cuda")
            nxt, ids = torch.empty(B, dtype=torch.int32, device="cuda"), torch.zeros(B, 1024, dtype=torch.long, device="cuda")
            logp, fin = torch.empty(B, device="cuda"), torch.full((B,), -1, dtype=torch.int32, device="cuda")
            eos_t = torch.tensor(eos, dtype=torch.int32, device="cuda")
            hist = torch.randint(0, V, (B, 1024), generator=gen, device="cuda")

            def torch_select():
                n = torch.multinomial(sampling_filter(logits, T, k, p).softmax(-1), 1, generator=gen).squeeze(1)
                n = torch.where(unf_t, n, torch.full_like(n, 0))
                u = unf_t
                for e in eos:
                    u = u & (n != e)
                return n, u

            def device_select(pen=1.0):
                unf.fill_(1)
                hip.call("vlr_sample_tokens", logits, B, V, V, 1, T, k, p, pen, hist, 1000 if pen != 1.0 else 0, 1024, 1, hist,
                         1024, 24 if pen != 1.0 else 0, eos_t, 1, 0, 1234, 0, 7, None, unf, nxt, ids, 1024, logp, fin, None)

            t = dict(torch=[], device=[], penalty=[], copy=[])
            for r in range(WARM + REPS):
                a = _ev()
                torch_select()
                b = _ev()
                device_select()
                c = _ev()
                device_select(1.1)
                d = _ev()
                dst.copy_(logits)
                e = _ev()
                torch.cuda.synchronize()
                if r >= WARM:
                    for name, (s_, e_) in (("torch", (a, b)), ("device", (b, c)), ("penalty", (c, d)), ("copy", (d, e))):
                        t[name].append(s_.elapsed_time(e_))
            lines.append(f"B={B:2d} V={V:6d} T={T} top_k={k:2d} top_p={p}:")
            lines.append(f"    torch ops (filter, softmax, multinomial, where, eos)      {_fmt(t['torch'])}")
            lines.append(f"    vlr_sample_tokens (incl. the 1-launch reset of the flags)  {_fmt(t['device'])}")
            lines.append(f"    vlr_sample_tokens + repetition_penalty 1.1, 1024 ids       {_fmt(t['penalty'])}")
            lines.append(f"    device copy of the logits ({B * V * 4 / 1e6:6.2f} MB read + written)    {_fmt(t['copy'])}")


def generate(a, lines):
    from vlrlhf.models.Llava import LlavaForRL
    from vlrlhf.utils.synthetic import LLAVA_1_5_7B, init_random_model, synthetic_batch
    cfg = dict(LLAVA_1_5_7B, layers=a.layers)
    model = LlavaForRL(cfg)
    init_random_model(model, seed=0, std=0.02, policy_delta=1e-3)
    model.apply_lora(dict(r=64, lora_alpha=16, lora_dropout=0.0, target_modules="auto", bias="none", seed=0))
    model.eval()
    P, G = a.prompts, a.generations
    b = synthetic_batch(P, 2 * a.new, cfg["image_token"], 32000, cfg["image_size"], seed=1234)
    lab = b["chosen_labels"]
    p = int((lab[0] != -100).nonzero()[0])
    ids = b["chosen_input_ids"][:, :p].cuda()
    kw = dict(input_ids=ids, attention_mask=torch.ones_like(ids), pixel_values=b["img_input_dict"]["pixel_values"].cuda(), do_sample=True,
              num_return_sequences=G, max_new_tokens=a.new, eos_token_id=cfg["vocab"] - 1, pad_token_id=0, use_cache=True, merge_lora=False)
    gen = torch.Generator(device="cuda").manual_seed(5)

    def run(sampler):
        s = _ev()
        out = model.generate(sampler=sampler, **(dict(generator=gen) if sampler == "torch" else dict(seed=5)), **kw)
        e = _ev()
        torch.cuda.synchronize()
        assert out.shape == (P * G, p + a.new), out.shape
        return s.elapsed_time(e)
    run("torch"), run("device")                               # warm-up: buffers, the first launches
    t = dict(torch=[], device=[])
    for _ in range(a.blocks):
        for name in ("torch", "device"):
            t[name].append(run(name))
    lines.append(f"generate: {P} prompts x {G} samples = {P * G} rows, {p} query tokens + a 336^2 image, {a.new} new tokens, {a.layers} layers, "
                 f"LLaVA-1.5-7B widths, LoRA r 64 live, shared prompt cache, top_k 50 / top_p 1 / T 1; {a.blocks} alternating blocks after one warm-up each")
    for name in ("torch", "device"):
        v = t[name]
        lines.append(f"    sampler={name:6s}  blocks {', '.join(f'{x:8.1f}' for x in v)} ms   median {statistics.median(v):8.1f} ms = "
                     f"{statistics.median(v) / a.new:6.3f} ms per new token   spread {min(v):8.1f} .. {max(v):8.1f}")
    d = statistics.median(t["torch"]) - statistics.median(t["device"])
    lines.append(f"    torch - device: {d:8.1f} ms per call = {d / a.new * 1e3:7.1f} us per new token "
                 f"(block-to-block spread: torch {max(t['torch']) - min(t['torch']):.1f} ms, device {max(t['device']) - min(t['device']):.1f} ms)")


def main():
    ap = argparse.ArgumentParser()
    for k, v in dict(layers=32, prompts=4, generations=8, new=256, blocks=3).items():
        ap.add_argument(f"--{k}", type=int, default=v)
    ap.add_argument("--skip_generate", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_sampler.txt"))
    a = ap.parse_args()
    lines = [f"# tools/sampler_bench.py {time.strftime('%Y-%m-%d')}, {torch.cuda.get_device_name(0)}: the per-token selection alone, three-way "
             f"alternating (HIP events, medians of {REPS} after {WARM} warm-up rounds)"]
    with torch.no_grad():
        selection(lines)
        if not a.skip_generate:
            generate(a, lines)
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
