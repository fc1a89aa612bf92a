#!/usr/bin/env python3
"""generate() with active LoRA adapters on the MI355X: what decoding with LIVE adapters costs against the merged copy, measured.

    python tools/decode_lora_bench.py [--out profiles/decode_live_lora.txt] [--layers 32] [--new 48] [--rank 128]

LLaVA-1.5-7B shapes, 4 prompts of 1024 tokens + a 336^2 image, adapters of rank --rank on the seven decoder linears (random, non-zero).
Two measurements, each in a process of its own under its own time limit; the driver stops at the first one that fails:
  bf16    ms per new token of (a) engine.decode_step with live adapters on the policy, (b) decode_step on merged weights - plus the
          one-off engine.merged_weights() time and the HBM it takes - and (c) the re-forward loop (one whole forward per token, live
          adapters).  (a), (b) and (c) alternate inside one process: same clocks, same neighbours.
  packed  (d) decode_step with live adapters over a packed GPTQ int4 base (nothing can be merged there)
The yardstick for (a) is (b): the merged decode runs the adapter-free kernels.  The launches per decoder layer in the output are NOT
counted in the run: they are read from the layer driver (csrc/layers.cpp layer_decode: 13 adapter-free, 17 with four live adapters -
one x A^T launch each) and the field's name says so; update LAUNCHES with the driver.
Times are HIP events on the launch stream, medians over the steps.  Weights are random: no kernel here is data dependent."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vl-rlhf_amd"))
sys.path.insert(0, ROOT)

LIMITS = dict(bf16=540, packed=420)                                          # seconds per measurement
G = 128
LAUNCHES = dict(adapter_free=13, live_adapters=17)


def ev():
    import torch
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


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
                K, N = shape[1], shape[0]
                eng.packed[name] = gptq.PackedLinear(torch.randint(-2 ** 31, 2 ** 31 - 1, (K // 8, N), dtype=torch.int32, device=eng.dev),
                                                     torch.randint(-2 ** 31, 2 ** 31 - 1, (K // G, N // 8), dtype=torch.int32, device=eng.dev),
                                                     (torch.rand(K // G, N, device=eng.dev) * 0.004 + 0.0005).half(), G)
    init_random_model(model, seed=0, std=0.02)
    model.apply_lora(dict(r=a.rank, lora_alpha=16, lora_dropout=0.0, target_modules="auto", bias="none"))
    g = torch.Generator(device=eng.dev).manual_seed(5)
    for v in eng.lv.values():
        v.copy_((torch.randn(v.shape, generator=g, device=eng.dev) * 0.01).to(v.dtype))
    model.eval()
    torch.cuda.synchronize()
    return cfg, model


def prompts(cfg, eng):
    from vlrlhf.utils.synthetic import synthetic_batch
    batch = synthetic_batch(4, 1024, cfg["image_token"], 32000, cfg["image_size"], seed=1234, prompt_frac=1.0)
    return (batch["prompt_input_ids"].to(eng.dev), batch["prompt_attention_mask"].to(eng.dev), batch["img_input_dict"]["pixel_values"].to(eng.dev))


def prefill(model, ws, ids, mask, pv, new):
    eng = model.engine
    cache = eng.new_kv_cache(ids.shape[0], new + 1)
    c = eng.forward_hidden(ws, ids, mask, None, pv, save=False, tag="policy_ng", kv_cache=cache)
    return cache, model._last_logits(c, ids.shape[0], ws.v["lm_head"]).argmax(-1), c["S"]


def bf16(a):
    import torch
    cfg, model = build_model(a, False)
    eng = model.engine
    ids, mask, pv = prompts(cfg, eng)
    with torch.no_grad():
        free0 = torch.cuda.mem_get_info()[0]
        s = ev()
        merged = eng.merged_weights()
        e = ev()
        torch.cuda.synchronize()
        merge_ms, merged_gb = s.elapsed_time(e), (free0 - torch.cuda.mem_get_info()[0]) / 1e9
        live_cache, tok_l, S = prefill(model, eng.policy, ids, mask, pv, a.new)
        merged_cache, tok_m, _ = prefill(model, merged, ids, mask, pv, a.new)
        t = dict(live=[], merged=[], reforward=[])
        kw = dict(input_ids=ids, attention_mask=mask, pixel_values=pv, do_sample=False, pad_token_id=0, eos_token_id=10 ** 6, use_cache=False)
        for i in range(a.new):                   # the cases alternate: same clocks, same neighbours
            s = ev()
            tok_l = eng.decode_step(eng.policy, tok_l, live_cache).argmax(-1)
            m = ev()
            tok_m = eng.decode_step(merged, tok_m, merged_cache).argmax(-1)
            e = ev()
            torch.cuda.synchronize()
            t["live"].append(s.elapsed_time(m))
            t["merged"].append(m.elapsed_time(e))
            if i % 8 == 7:                       # the re-forward loop: two tokens per sample, the second (vision features cached) is timed
                s = ev()
                model.generate(max_new_tokens=1, **kw)
                m = ev()
                model.generate(max_new_tokens=2, **kw)
                e = ev()
                torch.cuda.synchronize()
                t["reforward"].append(m.elapsed_time(e) - s.elapsed_time(m))
    med = {k: statistics.median(v[8:] if k != "reforward" else v) for k, v in t.items()}
    return dict(bf16=dict(layers=eng.L, rank=a.rank, prompts=4, merged_rows=S,
                          a_live_ms_per_token=round(med["live"], 3), b_merged_ms_per_token=round(med["merged"], 3),
                          b_merge_once_ms=round(merge_ms, 1), b_merged_copy_GB=round(merged_gb, 2), c_reforward_ms_per_token=round(med["reforward"], 2),
                          live_over_merged=round(med["live"] / med["merged"], 3), launches_per_layer_read_from_layers_cpp=LAUNCHES))


def packed(a):
    import torch
    cfg, model = build_model(a, True)
    eng = model.engine
    ids, mask, pv = prompts(cfg, eng)
    with torch.no_grad():
        cache, tok, S = prefill(model, eng.policy, ids, mask, pv, a.new)
        t = dict(live=[], plain=[])
        for lora, key in ((None, "live"), (False, "plain")):
            for _ in range(a.new // 2):
                s = ev()
                tok = eng.decode_step(eng.policy, tok, cache, lora=lora).argmax(-1)
                e = ev()
                torch.cuda.synchronize()
                t[key].append(s.elapsed_time(e))
    med = {k: statistics.median(v[4:]) for k, v in t.items()}
    return dict(packed=dict(layers=eng.L, rank=a.rank, group=G, merged_rows=S, d_live_ms_per_token=round(med["live"], 3),
                            adapters_off_ms_per_token=round(med["plain"], 3), live_over_adapters_off=round(med["live"] / med["plain"], 3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", choices=["", "bf16", "packed"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_live_lora.txt"))
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--new", type=int, default=48)
    ap.add_argument("--rank", type=int, default=128)
    a = ap.parse_args()
    if a.only:                                   # one measurement, in this process
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("decode_lora_bench.py measures on the MI355X: no GPU here")
        res = dict(bf16=bf16, packed=packed)[a.only](a)
        res["device"] = torch.cuda.get_device_name(0)
        print("RESULT " + json.dumps(res))
        return
    lines = []
    for name in ("bf16", "packed"):              # chained: a failure (or a time limit) ends the run, nothing else is started
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--only", name, "--layers", str(a.layers),
               "--new", str(a.new), "--rank", str(a.rank)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        res = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"decode_lora_bench.py: {name} failed with status {r.returncode}; stopping")
        lines.append(json.dumps(json.loads(res[-1][len("RESULT "):]), indent=1))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# tools/decode_lora_bench.py: ms per new token - (a) live adapters, (b) merged weights, (c) re-forward loop, (d) packed base + live adapters\n"
                + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
