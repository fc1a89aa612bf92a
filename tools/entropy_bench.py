#!/usr/bin/env python3
"""What the policy entropy costs on the MI355X, written to profiles/lmhead_entropy.txt:
    python tools/entropy_bench.py [--rows 8192] [--reps 12] [--prompts 4] [--generations 8] [--text_len 512] [--mini 8] [--steps 3]
                                  [--warmup 1] [--layers 32] [--skip_step] [--margins FILE] [--out profiles/lmhead_entropy.txt]
0. the registers of the two new instantiations of gemm256p_kernel (fuse 8 | 9) beside fuse 4 | 5, from the assembly the build keeps
   (vl-rlhf_amd/build/gemm256p-hip-amdgcn-amd-amdhsa-gfx950.s), when it is there.
1. vlr_lmhead_logps_entropy_fwd against vlr_lmhead_logps_fwd and vlr_lmhead_logps_entropy_bwd against vlr_lmhead_logps_bwd (nseq = R),
   `rows` rows at (V, H) = (32000, 4096) and (151936, 4096): the calls alternate in one process, so both see the same clocks and the same
   neighbours; HIP events around 3 back-to-back calls, medians over `reps` rounds.  The yardstick is the existing kernel of the same run.
2. one GRPO step (VLGRPOTrainer.step on fixed random responses: no generate, no reward model) at the configuration of profiles/grpo.txt -
   LLaVA-1.5-7B widths, LoRA r 64, 4 prompts x 8 samples x 512 text tokens, mini_batch_size 8 x 4 accumulated, beta 0.04 - with
   log_entropy off and on, on the SAME trainer in alternating blocks of `steps` steps.
--margins FILE appends the parity figures recorded by VLR_ENTROPY_MARGINS=FILE python -m pytest tests/test_hip_entropy.py -m gpu -s."""
import argparse
import os
import re
import statistics
import sys
import time

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


def registers():
    path = os.path.join(ROOT, "vl-rlhf_amd", "build", "gemm256p-hip-amdgcn-amd-amdhsa-gfx950.s")
    if not os.path.exists(path):
        say("registers: the build's assembly is not here (vl-rlhf_amd/build/): not reported")
        return
    text = open(path).read()
    say("gemm256p_kernel<NT, continuous, FUSE> from the build's assembly: fuse 4 / 5 the existing lm-head epilogues, 8 / 9 the entropy ones")
    for fuse in (4, 8, 5, 9):
        name = r"_Z15gemm256p_kernelILb0ELb0ELi0ELb1ELi%dELb0ELb0ELb0ELb0EE\w+" % fuse
        m = re.search(r"\.agpr_count:\s+(\d+)\n(?:(?!\.agpr_count:).)*?\.name:\s+" + name + r"\n.*?\.private_segment_fixed_size:\s+(\d+)\n.*?"
                      r"\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text, re.S)      # (the metadata's keys are in alphabetical order)
        if not m:
            say(f"  fuse {fuse}: not found")
            continue
        say(f"  fuse {fuse}: {m.group(3)} VGPRs + {m.group(1)} AGPRs, {m.group(4)} spilled, scratch {m.group(2)} B/lane")


def kernels(a):
    from vlrlhf import _hip as hip
    R = a.rows
    g = torch.Generator(device="cuda").manual_seed(0)
    for V, H in ((32000, 4096), (151936, 4096)):
        hg = (torch.randn(R, H, generator=g, device="cuda")).bfloat16()
        w = (torch.randn(V, H, generator=g, device="cuda") * 0.02).bfloat16()
        tgt = torch.randint(0, V, (R,), generator=g, device="cuda", dtype=torch.int32)
        assert hip.helper("vlr_lmhead_is_fused", R, V, H)
        ws = torch.empty(int(hip.lib().vlr_lmhead_workspace_bytes(R, V)), dtype=torch.uint8, device="cuda")
        ews = torch.empty(int(hip.lib().vlr_lmhead_entropy_workspace_bytes(R, V)), dtype=torch.uint8, device="cuda")
        tok, lse, ent = (torch.empty(R, device="cuda") for _ in range(3))
        dl = torch.empty(R, V, dtype=torch.bfloat16, device="cuda")
        dlogp, dent = torch.randn(R, generator=g, device="cuda"), torch.randn(R, generator=g, device="cuda")
        so = torch.arange(R + 1, dtype=torch.int32, device="cuda")
        calls = {
            "vlr_lmhead_logps_fwd": lambda: hip.call("vlr_lmhead_logps_fwd", hg, w, tgt, tok, lse, ws, None, R, V, H),
            "vlr_lmhead_logps_entropy_fwd": lambda: hip.call("vlr_lmhead_logps_entropy_fwd", hg, w, tgt, tok, lse, ent, ews, None, R, V, H),
            "vlr_lmhead_logps_bwd": lambda: hip.call("vlr_lmhead_logps_bwd", hg, w, tgt, lse, so, R, dlogp, 0, dl, ws, None, R, V, H),
            "vlr_lmhead_logps_entropy_bwd": lambda: hip.call("vlr_lmhead_logps_entropy_bwd", hg, w, tgt, lse, ent, dlogp, dent, dl, ews, None, R, V, H),
        }
        calls["vlr_lmhead_logps_entropy_fwd"]()                # lse and entropy of the backward's inputs
        say(f"R = {R}, V = {V}, H = {H}: {2.0 * R * V * H / 1e12:.2f} TFLOP per call; workspace {ws.numel() / 1e6:.0f} MB (pairs) / {ews.numel() / 1e6:.0f} MB (triples)")
        for old, new in (("vlr_lmhead_logps_fwd", "vlr_lmhead_logps_entropy_fwd"), ("vlr_lmhead_logps_bwd", "vlr_lmhead_logps_entropy_bwd")):
            for f in (calls[old], calls[new]):
                event_ms(f, 2)
            t = {old: [], new: []}
            for _ in range(a.reps):
                for n in (old, new):
                    t[n].append(event_ms(calls[n], 3))
            for n in (old, new):
                med = statistics.median(t[n])
                say(f"  {n:30s} median {med:8.3f} ms  (min {min(t[n]):.3f}, max {max(t[n]):.3f})  {2.0 * R * V * H / med / 1e9:7.1f} TFLOP/s")
            say(f"  ratio {new} / {old} = {statistics.median(t[new]) / statistics.median(t[old]):.4f}; spread of the existing call over the rounds "
                f"(max - min) / median = {(max(t[old]) - min(t[old])) / statistics.median(t[old]):.4f}")
        del hg, w, dl, ws, ews
        torch.cuda.empty_cache()


def step(a):
    from vlrlhf.base.trainer import GRPOConfig
    from vlrlhf.models.Llava import LlavaForRL, LlavaGRPOTrainer
    from vlrlhf.utils.synthetic import LLAVA_1_5_7B, init_random_model, synthetic_batch
    cfg = dict(LLAVA_1_5_7B, layers=a.layers)
    P, G = a.prompts, a.generations
    N = P * G
    model = LlavaForRL(cfg)
    ref = init_random_model(model, seed=0, std=0.02, policy_delta=1e-3)
    del ref
    model.apply_lora(dict(r=64, lora_alpha=16, lora_dropout=0.0, target_modules="auto", bias="none", seed=0))
    tr = LlavaGRPOTrainer(GRPOConfig(batch_size=P, num_generations=G, mini_batch_size=a.mini, gradient_accumulation_steps=N // a.mini,
                                     learning_rate=1e-6, beta=0.04), model)
    b = synthetic_batch(P, a.text_len, cfg["image_token"], 32000, cfg["image_size"], seed=1234)
    ids, lab, px = b["chosen_input_ids"], b["chosen_labels"], b["img_input_dict"]["pixel_values"]
    p = int((lab[0] != -100).nonzero()[0])
    qs = [r[:p] for r in ids]
    gen = torch.Generator().manual_seed(5)
    responses = [torch.randint(3, 31000, (a.text_len - p,), generator=gen) for _ in range(N)]
    scores = torch.randn(N, generator=gen).tolist()

    def one():
        tr.step(qs, responses, scores, pixel_values=px)
    for _ in range(a.warmup):
        one()
    say(f"GRPO step (no generate, no scoring): {P} prompts x {G} samples = {N} rows x {a.text_len} text tokens ({p} query + {a.text_len - p} response "
        f"tokens), {a.layers} layers, LLaVA-1.5-7B widths, LoRA r 64, mini_batch_size {a.mini} x {N // a.mini} accumulated, beta 0.04")
    med = {False: [], True: []}
    for block in range(4):                       # off, on, off, on on the same trainer
        on = bool(block % 2)
        tr.config.log_entropy = on
        one()                                    # (one unmeasured step after the switch)
        ms = [event_ms(one, 1) for _ in range(a.steps)]
        med[on].append(statistics.median(ms))
        say(f"  log_entropy {str(on):5s} median {med[on][-1]:9.2f} ms  (min {min(ms):.2f}, max {max(ms):.2f}) over {a.steps} steps")
    off, on = statistics.mean(med[False]), statistics.mean(med[True])
    spread = max(abs(med[False][0] - med[False][1]), abs(med[True][0] - med[True][1]))
    say(f"  log_entropy on - off = {on - off:+.2f} ms ({(on - off) / off * 100:+.3f} %); block-to-block spread of one setting {spread:.2f} ms")


def main():
    p = argparse.ArgumentParser()
    for k, v in dict(rows=8192, reps=12, prompts=4, generations=8, text_len=512, mini=8, steps=3, warmup=1, layers=32).items():
        p.add_argument(f"--{k}", type=int, default=v)
    p.add_argument("--skip_step", action="store_true")
    p.add_argument("--margins", default=None)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "lmhead_entropy.txt"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("entropy_bench.py measures on the MI355X: no GPU here, nothing measured")
    say(f"# tools/entropy_bench.py {time.strftime('%Y-%m-%d')} --rows {a.rows} --reps {a.reps} --steps {a.steps} --layers {a.layers}  ({torch.cuda.get_device_name(0)})")
    registers()
    kernels(a)
    if not a.skip_step:
        step(a)
    if a.margins and os.path.exists(a.margins):
        say("")
        say("# parity (fixtures llava_hipsmall / qwenvl_small; tests/test_hip_entropy.py, VLR_ENTROPY_MARGINS): the measured logit deviation between "
            "the engine and the fp32 oracle is what the entropy tolerance is made of")
        with open(a.margins) as f:
            for ln in f:
                say(ln.rstrip("\n"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
