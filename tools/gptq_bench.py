#!/usr/bin/env python3
"""q_lora on the MI355X: what the packed int4 base costs and saves, measured.

    python tools/gptq_bench.py [--out profiles/gptq_q_lora.txt] [--layers 32] [--new 64] [--steps 3]

Three measurements, each in a process of its own under its own time limit; the driver stops at the first one that fails:
  kernels  vlr_gemv_w4 against vlr_gemv_bf16 at M = 4 and the four decoder projection shapes of LLaVA-1.5-7B (the first four of
           SHAPES_7B in tests/test_hip_decode_kernels.py), group size 128.  Weights cycle through copies totalling >= 1 GiB (bf16) so
           that no call is served from the 256 MiB Infinity Cache; the two kernels alternate inside one timed run.
  decode   ms per new token of the KV-cache decode (engine.decode_step after one prefill) on the 7B shapes, packed against bf16
  step     one LoRA DPO step (2 pairs x 1024 tokens + a 336^2 image, forward + reference forward + backward + AdamW) over the packed
           base against the same step over a bf16 base
Times are HIP events on the launch stream, medians over the repetitions.  Weights are random: no kernel here is data dependent."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vl-rlhf_amd"))
sys.path.insert(0, ROOT)

SHAPES_7B = [(4096, 12288), (4096, 4096), (4096, 22016), (11008, 4096)]      # (K, N): qkv, o, gate|up, down
LIMITS = dict(kernels=240, decode=420, step=420)                             # seconds per measurement
G = 128


def ev():
    import torch
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def random_packed(K, N, g, dev):
    import torch
    return (torch.randint(-2 ** 31, 2 ** 31 - 1, (K // 8, N), dtype=torch.int32, device=dev),
            torch.randint(-2 ** 31, 2 ** 31 - 1, (K // g, N // 8), dtype=torch.int32, device=dev),
            (torch.rand(K // g, N, device=dev) * 0.004 + 0.0005).half())


def kernels(a):
    import torch
    from vlrlhf import _hip
    dev, M, out = "cuda", 4, []
    for K, N in SHAPES_7B:
        copies = max(2, -(-(1 << 30) // (N * K * 2)))
        Ws = [torch.randn(N, K, device=dev).bfloat16() * 0.02 for _ in range(copies)]
        Qs = [random_packed(K, N, G, dev) for _ in range(copies)]
        X = torch.randn(M, K, device=dev).bfloat16()
        Y = torch.zeros(M, N, dtype=torch.bfloat16, device=dev)
        ws = torch.empty(max(int(_hip.lib().vlr_gemv_workspace_bytes(M, N, K)), int(_hip.lib().vlr_gemv_w4_workspace_bytes(M, N, K))),
                         dtype=torch.uint8, device=dev)
        bf = lambda i: _hip.call("vlr_gemv_bf16", 0, X, K, Ws[i], Y, N, None, None, 0, None, None, None, 0, 128, 0, M, N, K, ws)      # noqa: E731
        w4 = lambda i: _hip.call("vlr_gemv_w4", 0, X, K, *Qs[i], G, Y, N, None, None, 0, None, None, None, 0, 128, 0, M, N, K, ws)     # noqa: E731
        for f in (bf, w4):
            f(0), f(1)
        t = dict(bf16=[], w4=[])
        torch.cuda.synchronize()
        for rep in range(5):                     # the kernels alternate: same clocks, same neighbours
            for name, f in (("bf16", bf), ("w4", w4)):
                s = ev()
                for i in range(copies):
                    f(i)
                e = ev()
                torch.cuda.synchronize()
                t[name].append(s.elapsed_time(e) * 1e3 / copies)
        b, w = statistics.median(t["bf16"]), statistics.median(t["w4"])
        packed_bytes = N * K // 2 + (K // G) * N * 2 + (K // G) * N // 2
        out.append(dict(K=K, N=N, M=M, group=G, bf16_us=round(b, 2), w4_us=round(w, 2), w4_over_bf16=round(w / b, 3),
                        bf16_TBs=round(N * K * 2 / b / 1e6, 3), w4_packed_TBs=round(packed_bytes / w / 1e6, 3)))
        del Ws, Qs
    return dict(kernels=out)


def build_model(a, packed):
    import torch
    from vlrlhf import gptq
    from vlrlhf.models.Llava import LlavaForRL
    from vlrlhf.utils.synthetic import LLAVA_1_5_7B, init_random_model
    cfg = dict(LLAVA_1_5_7B, layers=a.layers)
    if packed:
        cfg["gptq"] = dict(bits=4, group_size=G)
    model = LlavaForRL(cfg)
    eng = model.engine
    if packed:
        for name, shape, _ in eng.layout.entries:
            if name in eng.layout.packed:
                eng.packed[name] = gptq.PackedLinear(*random_packed(shape[1], shape[0], G, eng.dev), G)
    init_random_model(model, seed=0, std=0.02)
    torch.cuda.synchronize()
    return cfg, model


def decode(a):
    import torch
    from vlrlhf.utils.synthetic import synthetic_batch
    out = {}
    for packed in (False, True):
        cfg, model = build_model(a, packed)
        model.eval()
        eng = model.engine
        batch = synthetic_batch(4, 1024, cfg["image_token"], 32000, cfg["image_size"], seed=1234, prompt_frac=1.0)
        ids, mask = batch["prompt_input_ids"].to(eng.dev), batch["prompt_attention_mask"].to(eng.dev)
        pv = batch["img_input_dict"]["pixel_values"].to(eng.dev)
        with torch.no_grad():
            cache = eng.new_kv_cache(ids.shape[0], a.new + 1)
            s0 = ev()
            c = eng.forward_hidden(model.weights, ids, mask, None, pv, save=False, tag="policy_ng", kv_cache=cache)
            tok = model._last_logits(c, ids.shape[0], model.weights.v["lm_head"]).argmax(-1)
            e0 = ev()
            steps = []
            for _ in range(a.new):
                s = ev()
                tok = eng.decode_step(model.weights, tok, cache).argmax(-1)
                steps.append((s, ev()))
            torch.cuda.synchronize()
        ms = [x.elapsed_time(y) for x, y in steps][8:]
        out["packed" if packed else "bf16"] = dict(prefill_ms=round(s0.elapsed_time(e0), 2), decode_ms_per_token=round(statistics.median(ms), 3),
                                                   decode_ms_min=round(min(ms), 3), merged_rows=c["S"], layers=eng.L,
                                                   decoder_weight_GB=round((eng.packed_nbytes() if packed else eng.L * (eng.Nqkv * eng.H + eng.H * eng.Nq + 3 * eng.I * eng.H) * 2) / 1e9, 3))
        del model, cache, c
        torch.cuda.empty_cache()
    out["packed_over_bf16"] = round(out["packed"]["decode_ms_per_token"] / out["bf16"]["decode_ms_per_token"], 3)
    return dict(decode=out)


def step(a):
    import torch
    from types import SimpleNamespace
    from vlrlhf.models.Llava import LlavaDPOTrainer
    from vlrlhf.utils.synthetic import synthetic_batch
    out = {}
    for packed in (False, True):
        cfg, model = build_model(a, packed)
        args = SimpleNamespace(gradient_accumulation_steps=1, per_device_train_batch_size=2, learning_rate=1e-5, adam_beta1=0.9, adam_beta2=0.98,
                               adam_epsilon=1e-6, weight_decay=0.05, max_grad_norm=1.0, seed=0)
        tr = LlavaDPOTrainer(model, None, 0.1, 0, "sigmoid", args, None, -100, 0, "keep_end", None, None, None,
                             peft_config=dict(r=64, lora_alpha=16, lora_dropout=0.05, target_modules="auto", bias="none", seed=0))
        eng = model.engine
        eng.gradient_checkpointing = True
        batch = tr._prepare_inputs(synthetic_batch(2, 1024, cfg["image_token"], 32000, cfg["image_size"], seed=1234))
        eng.init_optimizer()
        model.train()
        ms = []
        for i in range(a.steps + 1):
            s = ev()
            tr.training_step(model, batch)
            eng.optimizer_step(1e-5, 0.9, 0.98, 1e-6, 0.05, 1.0)
            e = ev()
            torch.cuda.synchronize()
            if i:
                ms.append(s.elapsed_time(e))
        out["q_lora" if packed else "lora"] = dict(step_ms=round(statistics.median(ms), 2), step_ms_min=round(min(ms), 2), layers=eng.L,
                                                   peak_GB=round(torch.cuda.max_memory_allocated() / 1e9, 2))
        del model, tr
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
    out["q_lora_over_lora"] = round(out["q_lora"]["step_ms"] / out["lora"]["step_ms"], 3)
    return dict(step=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", choices=["", "kernels", "decode", "step"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gptq_q_lora.txt"))
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    if a.only:                                   # one measurement, in this process
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("gptq_bench.py measures on the MI355X: no GPU here")
        res = dict(kernels=kernels, decode=decode, step=step)[a.only](a)
        res["device"] = torch.cuda.get_device_name(0)
        print("RESULT " + json.dumps(res))
        return
    lines = []
    for name in ("kernels", "decode", "step"):   # chained: a failure (or a time limit) ends the run, nothing else is started
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--only", name, "--layers", str(a.layers),
               "--new", str(a.new), "--steps", str(a.steps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        res = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"gptq_bench.py: {name} failed with status {r.returncode}; stopping")
        lines.append(json.dumps(json.loads(res[-1][len("RESULT "):]), indent=1))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# tools/gptq_bench.py: vlr_gemv_w4 vs vlr_gemv_bf16, decode ms / token packed vs bf16, q_lora step vs lora step\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
