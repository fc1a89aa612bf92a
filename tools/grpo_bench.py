#!/usr/bin/env python3
"""Times the GRPO kernels and one GRPO step beside a PPO step of the same number of rows, and appends the figures to profiles/grpo.txt:
    python tools/grpo_bench.py [--prompts 4] [--generations 8] [--text_len 512] [--mini 8] [--steps 2] [--warmup 1] [--layers 32] [--skip_step]
                               [--margins FILE] [--out profiles/grpo.txt]
Kernels: vlr_grpo_advantages and vlr_grpo_loss alone (32 and 64 sequences of 256 / 512 response tokens), each alternating launch by launch
with a device-to-device copy that moves the same HBM traffic - clocks and co-tenants drift over both alike - HIP events around every
launch, medians reported.
Step: LLaVA-1.5-7B widths, LoRA r 64, random weights, P prompts of text_len / 2 query tokens, G samples of text_len / 2 new tokens each
from ONE generate call over the shared prompt cache, mini_batch_size `mini`, gradient accumulation over all P * G rows (one optimizer
step, so no old-log-prob pass), beta 0.04 (an adapter-off reference pass): HIP events around VLGRPOTrainer.generate, the reward model's
score over the P * G rows, and inside step() the no-grad passes and the optimisation.  The yardstick, from the same process: a PPO step
of P * G rows (P * G prompts, one sample each; the same minibatches, ppo_epochs 1), timed the way tools/ppo_bench.py times it.
--margins FILE appends the parity figures recorded by VLR_GRPO_MARGINS=FILE python -m pytest tests/test_hip_grpo.py -m gpu -s."""
import argparse
import gc
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vl-rlhf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ppo_bench import _alternate  # noqa: E402


def kernels(lines):
    from vlrlhf import _hip as hip
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")      # noqa: E731
    for P, G in ((4, 8), (64, 8), (64, 64)):
        sc, adv, st = rnd(P * G), torch.empty(P * G, device="cuda"), torch.empty(4, device="cuda")
        k, c = _alternate(lambda: hip.call("vlr_grpo_advantages", sc, P, G, 1, adv, st), 2 * P * G * 4)
        lines.append(f"vlr_grpo_advantages P={P:3d} G={G:3d}                 {k * 1e3:9.1f} us   copy moving {2 * P * G * 4 / 1e6:8.4f} MB {c * 1e3:9.1f} us")
    for n, L in ((32, 256), (64, 512)):
        R = n * L
        logp = -torch.rand(R, generator=g, device="cuda") * 3
        old, ref, adv = logp + 0.1 * rnd(R), logp + 0.1 * rnd(R), rnd(n)
        so = torch.arange(n + 1, dtype=torch.int32, device="cuda") * L
        dl, st = torch.empty(R, device="cuda"), torch.empty(8, device="cuda")
        for name, o, r, beta, traffic in (("old + ref, beta 0.04", old, ref, 0.04, 4), ("NULL old, beta 0", None, None, 0.0, 2)):
            k, c = _alternate(lambda: hip.call("vlr_grpo_loss", logp, o, r, adv, so, R, n, 0.2, 0.2, beta, 0, 0, 1.0, dl, st), traffic * R * 4)
            lines.append(f"vlr_grpo_loss       n={n:3d} R={R:6d} {name:22s}{k * 1e3:9.1f} us   copy moving {traffic * R * 4 / 1e6:8.4f} MB {c * 1e3:9.1f} us")


def _timed(fn):
    s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s_.record()
    out = fn()
    e_.record()
    torch.cuda.synchronize()
    return out, s_.elapsed_time(e_)


def _report(lines, rows):
    for name, v in rows:
        lines.append(f"{name:66s} median {statistics.median(v):9.2f} ms   min {min(v):9.2f}   max {max(v):9.2f}")


def step(a, lines):
    from vlrlhf.base.trainer import GRPOConfig, PPOConfig
    from vlrlhf.models.Llava import (LlavaForPPO, LlavaForRL, LlavaForRM, LlavaGRPOTrainer, LlavaPPOTrainer, LlavaRewardModel,
                                     LlavaWithValueHead)
    from vlrlhf.utils.synthetic import LLAVA_1_5_7B, init_random_model, synthetic_batch
    cfg = dict(LLAVA_1_5_7B, layers=a.layers)
    P, G = a.prompts, a.generations
    N = P * G
    lora = dict(r=64, lora_alpha=16, lora_dropout=0.0, target_modules="auto", bias="none", seed=0)
    rm_base = LlavaForRM(cfg)
    del_ref = init_random_model(rm_base, seed=1, std=0.02, policy_delta=1e-3)
    del del_ref
    rm = LlavaRewardModel(rm_base, seed=0)
    rm.eval()

    def queries(n):
        b = synthetic_batch(n, a.text_len, cfg["image_token"], 32000, cfg["image_size"], seed=1234)
        ids, lab = b["chosen_input_ids"], b["chosen_labels"]
        p = int((lab[0] != -100).nonzero()[0])
        return [r[:p] for r in ids], b["img_input_dict"]["pixel_values"], p

    def score(qs, responses, px):
        out = []
        for lo in range(0, len(qs), a.mini):
            q_, r_ = qs[lo:lo + a.mini], responses[lo:lo + a.mini]
            lens = [q.numel() + r.numel() for q, r in zip(q_, r_)]
            ids = torch.zeros(len(q_), max(lens), dtype=torch.long)
            mask = torch.zeros_like(ids)
            for i, (q, r) in enumerate(zip(q_, r_)):
                ids[i, :lens[i]], mask[i, :lens[i]] = torch.cat([q, r.cpu()]), 1
            out.append(rm.score(ids.cuda(), mask.cuda(), reward_cols=torch.tensor([n - 1 for n in lens]), pixel_values=px[lo:lo + a.mini].cuda()))
        return torch.cat(out)

    # ---- GRPO: P prompts, G samples each
    model = LlavaForRL(cfg)
    del_ref = init_random_model(model, seed=0, std=0.02, policy_delta=1e-3)
    del del_ref
    model.apply_lora(lora)
    tr = LlavaGRPOTrainer(GRPOConfig(batch_size=P, num_generations=G, mini_batch_size=a.mini, gradient_accumulation_steps=N // a.mini,
                                     learning_rate=1e-6, beta=0.04), model)
    tr.time_phases = True
    qs, px, p = queries(P)
    new = a.text_len - p
    gen_kw = dict(max_new_tokens=new, eos_token_id=cfg["vocab"] - 1, pad_token_id=0, use_cache=True)      # no row ends early
    gen, sc, ng, opt = [], [], [], []
    for k in range(a.warmup + a.steps):
        responses, t_gen = _timed(lambda: tr.generate(qs, generation_kwargs=gen_kw, pixel_values=px))
        scores, t_sc = _timed(lambda: score(tr._expand_queries(qs), responses, px.repeat_interleave(G, 0)))
        tr.step(qs, responses, scores.tolist(), pixel_values=px)
        if k >= a.warmup:
            gen.append(t_gen)
            sc.append(t_sc)
            ng.append(tr.last_timing["nograd_ms"])
            opt.append(tr.last_timing["optimisation_ms"])
    S = a.text_len + (cfg["image_size"] // cfg["patch_size"]) ** 2 - 1
    lines.append(f"GRPO step: {P} prompts x {G} samples = {N} rows x {a.text_len} text tokens (S = {S}: {p} query tokens, {new} sampled response tokens "
                 f"each, one generate call, shared prompt cache, live adapters), {a.layers} layers, LLaVA-1.5-7B widths, LoRA r 64, mini_batch_size "
                 f"{a.mini} x {N // a.mini} accumulated, num_iterations 1, beta 0.04, {a.steps} timed after {a.warmup} warm-up")
    _report(lines, (("generate (P prefills + one decode step of P * G rows per new token)", gen), ("score (the reward model on the P * G rows)", sc),
                    ("no-grad passes (adapter-off reference; no old-log-prob pass) + advantages", ng),
                    ("optimisation (forward, loss, backward per minibatch; one Adam step)", opt)))
    grpo_total = sum(statistics.median(v) for v in (gen, sc, ng, opt))
    del tr, model
    gc.collect()
    torch.cuda.empty_cache()
    # ---- the yardstick: a PPO step of N rows (N prompts, one sample each)
    base = LlavaForPPO(cfg)
    del_ref = init_random_model(base, seed=0, std=0.02, policy_delta=1e-3)
    del del_ref
    pmodel = LlavaWithValueHead(base, v_head_init_strategy="normal", seed=0)
    pmodel.apply_lora(lora)
    ptr = LlavaPPOTrainer(PPOConfig(batch_size=N, mini_batch_size=a.mini, gradient_accumulation_steps=N // a.mini, ppo_epochs=1, learning_rate=1e-6), pmodel)
    ptr.time_phases = True
    qs, px, p = queries(N)
    gen_kw = dict(gen_kw, do_sample=True)
    gen, sc, ro, opt = [], [], [], []
    for k in range(a.warmup + a.steps):
        responses, t_gen = _timed(lambda: ptr.generate(qs, generation_kwargs=gen_kw, batch_size=32, pixel_values=px))
        scores, t_sc = _timed(lambda: score(qs, responses, px))
        ptr.step(qs, responses, scores.tolist(), pixel_values=px)
        if k >= a.warmup:
            gen.append(t_gen)
            sc.append(t_sc)
            ro.append(ptr.last_timing["rollout_ms"])
            opt.append(ptr.last_timing["optimisation_ms"])
    lines.append(f"PPO step, the yardstick: {N} prompts x 1 sample = {N} rows of the same shape (generate in chunks of 32 rows), mini_batch_size {a.mini} x "
                 f"{N // a.mini} accumulated, ppo_epochs 1, {a.steps} timed after {a.warmup} warm-up")
    _report(lines, (("generate (N prefills + one decode step of N rows per new token)", gen), ("score (the reward model on the N rows)", sc),
                    ("rollout passes (policy + adapter-off reference + advantages)", ro),
                    ("optimisation (forward, loss, backward per minibatch; one Adam step)", opt)))
    ppo_total = sum(statistics.median(v) for v in (gen, sc, ro, opt))
    lines.append(f"sum of the four medians: GRPO {grpo_total:.2f} ms, PPO {ppo_total:.2f} ms per step of {N} rows")
    lines.append("(tokenising, decoding to text and image loading are host work and not timed here)")


def main():
    p = argparse.ArgumentParser()
    for k, v in dict(prompts=4, generations=8, text_len=512, mini=8, steps=2, warmup=1, layers=32).items():
        p.add_argument(f"--{k}", type=int, default=v)
    p.add_argument("--skip_step", action="store_true")
    p.add_argument("--margins", default=None)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "grpo.txt"))
    a = p.parse_args()
    lines = [f"# tools/grpo_bench.py {time.strftime('%Y-%m-%d')}, {torch.cuda.get_device_name(0)}: each kernel alone, alternating with a device copy moving the same bytes "
             "(read + write) (medians of 30 launches, HIP events)"]
    kernels(lines)
    if not a.skip_step:
        step(a, lines)
    if a.margins:
        lines.append("")
        lines.append("# parity (LLaVA fixture llava_hipsmall, Qwen-VL fixture qwenvl_small; 2 prompts x 2 samples, scores 1.0 / -0.5 / 0.25 / 2.0, beta 0.04, "
                     "epsilon 0.2 / 0.28, loss_type grpo)")
        with open(a.margins) as f:
            lines += [ln.rstrip("\n") for ln in f]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
