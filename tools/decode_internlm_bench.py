#!/usr/bin/env python3
"""InternLM-XComposer2 on the KV cache (InternLMXC2ForRL.enable_kv_cache) on the MI355X, measured against the re-forward loop.

    python tools/decode_internlm_bench.py [--out profiles/decode_internlm.txt] [--layers 32] [--rows 4] [--new 24]

One process under the driver's time limit: InternLM-XComposer2-VL-7B widths (hidden 4096, inter 14336, 32 heads over 8 K/V heads, PLoRA
r 256 on the image rows), `rows` prompts of one 490 px image (1225 patches) + 64 text tokens.  Twice - the full fine-tune weights, then
peft LoRA r 64 live over the frozen PLoRA decoder (merge_lora=False: how a policy samples inside training) -
  prefill      forward_hidden(kv_cache=...) of the prompts + the lm-head of the last rows: the cached route's one forward
  cached       ms per new token of engine.decode_step after that prefill (the first 4 steps dropped)
  re-forward   ms per new token of the loop a fresh model runs: generate of 2 tokens minus generate of 1 (vision features cached in both)
Times are HIP events on the launch stream, medians.  Weights are random: no kernel here is data dependent."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vl-rlhf_amd"))
sys.path.insert(0, ROOT)

LIMIT = 400                                                                  # seconds


def ev():
    import torch
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def measure(a):
    import torch
    from vlrlhf.models.InternLMXC2 import INTERNLM_XC2_VL_7B, InternLMXC2ForRL
    from vlrlhf.utils.synthetic import init_random_model, synthetic_batch
    cfg = dict(INTERNLM_XC2_VL_7B, layers=a.layers)
    model = InternLMXC2ForRL(cfg)
    eng = model.engine
    init_random_model(model, seed=0, std=0.02)
    model.eval()
    B = a.rows
    batch = synthetic_batch(B, 64, cfg["image_token"], 32000, cfg["image_size"], seed=1234, prompt_frac=1.0)
    ids, mask = batch["prompt_input_ids"].to(eng.dev), batch["prompt_attention_mask"].to(eng.dev)
    pv = batch["img_input_dict"]["pixel_values"].to(eng.dev)
    assert ids.shape[0] == B
    kw = dict(input_ids=ids, attention_mask=mask, pixel_values=pv, do_sample=False, pad_token_id=cfg["model_pad_token_id"], eos_token_id=10 ** 9,
              merge_lora=False)
    out = {}
    for route in ("full fine-tune weights", "peft LoRA r 64, live"):
        if route.startswith("peft"):
            model.apply_lora(dict(r=64, lora_alpha=64, lora_dropout=0.05, target_modules="auto", bias="none"))
            g = torch.Generator(device=eng.dev).manual_seed(5)
            for v in eng.lv.values():
                v.copy_((torch.randn(v.shape, generator=g, device=eng.dev) * 0.01).to(v.dtype))
            model.eval()
        model.enable_kv_cache()
        t = dict(prefill=[], cached=[], reforward=[])
        with torch.no_grad():
            for rep in range(3):
                cache = eng.new_kv_cache(B, a.new + 1)
                s = ev()
                c = eng.forward_hidden(model.weights, ids, mask, None, pv, save=False, tag="policy_ng", kv_cache=cache)
                tok = model._last_logits(c, B, model.weights.v["lm_head"]).argmax(-1).clamp(max=cfg["image_token"] - 1)
                e = ev()
                torch.cuda.synchronize()
                if rep:                                      # (the first pass allocates and evaluates the vision tower)
                    t["prefill"].append(s.elapsed_time(e))
            for i in range(a.new):
                s = ev()
                logits = eng.decode_step(model.weights, tok, cache)
                e = ev()
                torch.cuda.synchronize()
                tok = logits.argmax(-1).clamp(max=cfg["image_token"] - 1)
                if i >= 4:
                    t["cached"].append(s.elapsed_time(e))
            S = int(c["S"])
            del cache, c
            model.enable_kv_cache(False)
            for _ in range(3):                               # the re-forward loop: two tokens minus one
                s = ev()
                model.generate(max_new_tokens=1, **kw)
                m = ev()
                model.generate(max_new_tokens=2, **kw)
                e = ev()
                torch.cuda.synchronize()
                t["reforward"].append(m.elapsed_time(e) - s.elapsed_time(m))
        med = {k: statistics.median(v) for k, v in t.items()}
        out[route] = dict(prefill_ms=round(med["prefill"], 2), cached_ms_per_token=round(med["cached"], 3),
                          cached_spread_ms=[round(min(t["cached"]), 3), round(max(t["cached"]), 3)],
                          reforward_ms_per_token=round(med["reforward"], 2), reforward_spread_ms=[round(min(t["reforward"]), 2), round(max(t["reforward"]), 2)],
                          reforward_over_cached=round(med["reforward"] / med["cached"], 1), steps_timed={k: len(v) for k, v in t.items()})
    return dict(layers=eng.L, rows=B, merged_columns=S, routes=out)


def render(res):
    L = ["InternLM-XComposer2 on the KV cache against its re-forward loop, one MI355X (tools/decode_internlm_bench.py; random weights, HIP events,",
         "medians)", "",
         f"InternLM-XComposer2-VL-7B widths, {res['layers']} layers, {res['rows']} prompts of {res['merged_columns']} merged columns (one 490 px image = 1225 "
         "patches + 64 text tokens)", "",
         f"  {'route':<28}{'prefill ms':>12}{'cached ms/token':>18}{'(min - max)':>20}{'re-forward ms/token':>22}{'(min - max)':>20}{'re-forward / cached':>22}"]
    for name, r in res["routes"].items():
        L.append(f"  {name:<28}{r['prefill_ms']:>12}{r['cached_ms_per_token']:>18}{'(%s - %s)' % tuple(r['cached_spread_ms']):>20}"
                 f"{r['reforward_ms_per_token']:>22}{'(%s - %s)' % tuple(r['reforward_spread_ms']):>20}{r['reforward_over_cached']:>22}")
    L += ["", "  prefill: forward_hidden(kv_cache=...) + the lm-head of the last rows; cached: engine.decode_step, first 4 steps dropped;",
          "  re-forward: generate of 2 tokens minus generate of 1 on the loop a fresh model runs.  steps timed: "
          + str(next(iter(res["routes"].values()))["steps_timed"]), "", "device: " + res.get("device", "?")]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_internlm.txt"))
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--new", type=int, default=24, help="decode steps timed per route (the first 4 dropped)")
    a = ap.parse_args()
    if a.only:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("decode_internlm_bench.py measures on the MI355X: no GPU here")
        res = measure(a)
        res["device"] = torch.cuda.get_device_name(0)
        print("RESULT " + json.dumps(res))
        return
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--only", "--layers", str(a.layers), "--rows", str(a.rows),
           "--new", str(a.new)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    got = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not got:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"decode_internlm_bench.py failed with status {r.returncode}")
    res = json.loads(got[-1][len("RESULT "):])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(render(res))
    print(render(res))


if __name__ == "__main__":
    main()
