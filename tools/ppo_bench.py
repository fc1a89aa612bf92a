#!/usr/bin/env python3
"""Times the PPO kernels and one PPO step, and appends the figures to profiles/ppo.txt:
    python tools/ppo_bench.py [--rows 4] [--text_len 512] [--steps 4] [--warmup 1] [--layers 32] [--skip_step] [--out profiles/ppo.txt]
Kernels: vlr_ppo_advantages, vlr_ppo_loss and vlr_v_head_bwd alone at the reference recipe's sizes (64 sequences x 512 response tokens,
H = 4096), each alternating launch by launch with a device-to-device copy that moves the same HBM traffic (a copy of N bytes reads N and
writes N, so the copy is of half the kernel's bytes) - clocks and co-tenants drift over both alike - HIP events around every launch,
medians reported.
Step: LLaVA-1.5-7B widths, LoRA r 64, random weights, `rows` sequences of `text_len` text tokens (half query, half response; S =
text_len + 575), mini_batch_size = rows, ppo_epochs 1: HIP events around VLPPOTrainer.generate (sampling, live adapters, KV cache), the
reward model's score over query + response (a second set of 7B weights), and inside step() the rollout (policy and adapter-off reference
passes, advantages) and the optimisation (forward, loss, backward, Adam)."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vl-rlhf_amd"))


def _alternate(run, traffic, reps=30, warmup=5):
    """-> (median ms of run(), median ms of a device copy whose read + write is `traffic` bytes), launches alternating"""
    src = torch.empty(max(traffic // 2, 16), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    tk, tc = [], []
    for k in range(warmup + reps):
        for fn, acc in ((run, tk), (lambda: dst.copy_(src), tc)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            if k >= warmup:
                acc.append(s.elapsed_time(e))
    return statistics.median(tk), statistics.median(tc)


def kernels(lines):
    from vlrlhf import _hip as hip
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")      # noqa: E731
    for n, L in ((64, 512), (8, 512)):
        R = n * L
        old, ref, val, sc = rnd(R), rnd(R), rnd(R), rnd(n)
        so = torch.arange(n + 1, dtype=torch.int32, device="cuda") * L
        adv, ret, kls, st = torch.empty(R, device="cuda"), torch.empty(R, device="cuda"), torch.empty(n, device="cuda"), torch.empty(4, device="cuda")
        k, c = _alternate(lambda: hip.call("vlr_ppo_advantages", old, ref, val, so, sc, 0.2, 0, 1.0, 0.95, 0, adv, ret, kls, st, R, n), 5 * R * 4)
        lines.append(f"vlr_ppo_advantages  n={n:3d} R={R:6d}            {k * 1e3:9.1f} us   copy moving {5 * R * 4 / 1e6:8.2f} MB {c * 1e3:9.1f} us")
        dl, dv, st17 = torch.empty(R, device="cuda"), torch.empty(R, device="cuda"), torch.empty(17, device="cuda")
        k, c = _alternate(lambda: hip.call("vlr_ppo_loss", old, val, ref, val, adv, ret, R, 0.2, 0.2, 0.1, 10.0, 1.0, dl, dv, st17), 8 * R * 4)
        lines.append(f"vlr_ppo_loss        R={R:6d}                  {k * 1e3:9.1f} us   copy moving {8 * R * 4 / 1e6:8.2f} MB {c * 1e3:9.1f} us")
    H = 4096
    for R in (4096, 32768):
        hg, dhg = rnd(R, H).bfloat16(), rnd(R, H).bfloat16()
        w, gr = rnd(H).bfloat16(), rnd(R)
        dw, db = torch.zeros(H, dtype=torch.bfloat16, device="cuda"), torch.zeros(8, dtype=torch.bfloat16, device="cuda")
        ws = torch.empty(hip.lib().vlr_v_head_bwd_workspace_bytes(R, H), dtype=torch.uint8, device="cuda")
        k, c = _alternate(lambda: hip.call("vlr_v_head_bwd", hg, w, gr, dhg, dw, db, 0, ws, R, H), 3 * R * H * 2)
        lines.append(f"vlr_v_head_bwd      R={R:6d} H={H}            {k * 1e3:9.1f} us   copy moving {3 * R * H * 2 / 1e6:8.2f} MB {c * 1e3:9.1f} us"
                     f"   ({3 * R * H * 2 / k / 1e9:.2f} TB/s over hg + d hg read + d hg written)")


def step(a, lines):
    from vlrlhf.base.trainer import PPOConfig
    from vlrlhf.models.Llava import LlavaForPPO, LlavaPPOTrainer, LlavaWithValueHead
    from vlrlhf.utils.synthetic import LLAVA_1_5_7B, init_random_model, synthetic_batch
    cfg = dict(LLAVA_1_5_7B, layers=a.layers)
    base = LlavaForPPO(cfg)
    del_ref = init_random_model(base, seed=0, std=0.02, policy_delta=1e-3)
    del del_ref
    model = LlavaWithValueHead(base, v_head_init_strategy="normal", seed=0)
    model.apply_lora(dict(r=64, lora_alpha=16, lora_dropout=0.0, target_modules="auto", bias="none", seed=0))
    tr = LlavaPPOTrainer(PPOConfig(batch_size=a.rows, mini_batch_size=a.rows, ppo_epochs=1, learning_rate=1e-6), model)
    tr.time_phases = True
    b = synthetic_batch(a.rows, a.text_len, cfg["image_token"], 32000, cfg["image_size"], seed=1234)
    ids, lab = b["chosen_input_ids"], b["chosen_labels"]
    p = int((lab[0] != -100).nonzero()[0])
    qs = [r[:p] for r in ids]
    px = b["img_input_dict"]["pixel_values"]
    # the reward model that scores the samples: a second set of 7B weights with the reward head
    from vlrlhf.models.Llava import LlavaForRM, LlavaRewardModel
    rm_base = LlavaForRM(cfg)
    del_ref = init_random_model(rm_base, seed=1, std=0.02, policy_delta=1e-3)
    del del_ref
    rm = LlavaRewardModel(rm_base, seed=0)
    rm.eval()
    new = a.text_len - p
    gen_kw = dict(max_new_tokens=new, do_sample=True, eos_token_id=cfg["vocab"] - 1, pad_token_id=0, use_cache=True)      # no row ends early

    def timed(fn):
        s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s_.record()
        out = fn()
        e_.record()
        torch.cuda.synchronize()
        return out, s_.elapsed_time(e_)

    def score(responses):
        lens = [q.numel() + r.numel() for q, r in zip(qs, responses)]
        ids = torch.zeros(a.rows, max(lens), dtype=torch.long)
        mask = torch.zeros_like(ids)
        for i, (q, r) in enumerate(zip(qs, responses)):
            ids[i, :lens[i]], mask[i, :lens[i]] = torch.cat([q, r.cpu()]), 1
        return rm.score(ids.cuda(), mask.cuda(), reward_cols=torch.tensor([n - 1 for n in lens]), pixel_values=px.cuda())

    gen, sc, ro, opt = [], [], [], []
    for k in range(a.warmup + a.steps):
        responses, t_gen = timed(lambda: tr.generate(qs, generation_kwargs=gen_kw, pixel_values=px))
        scores, t_sc = timed(lambda: score(responses))
        tr.step(qs, responses, scores.tolist(), pixel_values=px)
        if k >= a.warmup:
            gen.append(t_gen)
            sc.append(t_sc)
            ro.append(tr.last_timing["rollout_ms"])
            opt.append(tr.last_timing["optimisation_ms"])
    S = a.text_len + (cfg["image_size"] // cfg["patch_size"]) ** 2 - 1
    lines.append(f"step: {a.rows} rows x {a.text_len} text tokens (S = {S}: {p} query tokens, {new} sampled response tokens each, live adapters, KV cache), "
                 f"{a.layers} layers, LLaVA-1.5-7B widths, LoRA r 64, mini_batch_size = rows, ppo_epochs 1, {a.steps} timed after {a.warmup} warm-up")
    for name, v in (("generate (prefill + one decode step per new token)", gen), ("score (the reward model on query + response)", sc),
                    ("rollout passes (policy + adapter-off reference + advantages)", ro), ("optimisation (forward, loss, backward, Adam)", opt)):
        lines.append(f"{name:62s} median {statistics.median(v):9.2f} ms   min {min(v):9.2f}   max {max(v):9.2f}")
    lines.append("(tokenising, decoding to text and image loading are host work and not timed here)")


def main():
    p = argparse.ArgumentParser()
    for k, v in dict(rows=4, text_len=512, steps=4, warmup=1, layers=32).items():
        p.add_argument(f"--{k}", type=int, default=v)
    p.add_argument("--skip_step", action="store_true")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo.txt"))
    a = p.parse_args()
    lines = [f"# tools/ppo_bench.py {time.strftime('%Y-%m-%d')}, {torch.cuda.get_device_name(0)}: each kernel alone, alternating with a device copy moving the same bytes (read + write) "
             "(medians of 30 launches, HIP events)"]
    kernels(lines)
    if not a.skip_step:
        step(a, lines)
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
