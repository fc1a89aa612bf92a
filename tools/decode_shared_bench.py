#!/usr/bin/env python3
"""generate(num_return_sequences=n) on the MI355X: n samples per prompt over ONE shared prompt K / V cache against the parent commit's
way of getting them - every prompt repeated n times in the batch of the existing cached route - measured.

    python tools/decode_shared_bench.py [--out profiles/decode_shared_prompt.txt] [--layers 32] [--new 40] [--fanouts 2,4,8] [--errors FILE]

Shapes built in memory (random weights: no kernel here is data dependent):
  llava7b   LLaVA-1.5-7B, 4 prompts of 1024 tokens + a 336^2 image = 1599 merged rows
  mistral   LLaVA-Next-Mistral-7B attention shapes (32 heads over 8 kv heads), 2 prompts x 4975 columns: the attention kernels alone
Each measurement runs in a process of its own under its own time limit; the driver stops at the first one that fails.  Per fan-out n:
  prefill ms (one pass of P prompts against one of P * n), ms per new token of engine.decode_step on the SharedPromptKVCache against
  decode_step on the KVCache of the repeated batch, bytes of K / V allocated by each, and the attention entry point alone
  (vlr_attn_decode_shared against vlr_attn_decode_gqa on the materialised cache, one layer's buffers).
The two routes ALTERNATE step by step inside one process: same clocks, same neighbours.  Times are HIP events on the launch stream; the
first 8 steps are warm-up, the medians and the spread (min .. max) of the rest are reported.  --errors FILE: lines of measured test errors
to carry into the profile file beside the timings."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vl-rlhf_amd"))
sys.path.insert(0, ROOT)

LIMITS = dict(llava7b=560, mistral=200)                                      # seconds per measurement
WARM = 8


def ev():
    import torch
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def stats(v):
    v = v[WARM:] if len(v) > 2 * WARM else v
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), n=len(v))


def attn_alone(P, n, nh, nkv, Lp, Lt, reps=60):
    """vlr_attn_decode_shared against vlr_attn_decode_gqa on the materialised cache, one layer's buffers, alternating -> ms each"""
    import torch
    from vlrlhf import _hip
    dev, hd, B = "cuda", 128, P * n
    Hq = nh * hd
    bf = torch.bfloat16
    kp, vp = torch.randn(P, nkv, Lp, hd, device=dev).to(bf), torch.randn(P, nkv, Lp, hd, device=dev).to(bf)
    kt, vt = torch.randn(B, nkv, Lt, hd, device=dev).to(bf), torch.randn(B, nkv, Lt, hd, device=dev).to(bf)
    km = torch.ones(P, Lp, dtype=torch.int32, device=dev)
    kc = torch.cat([kp.repeat_interleave(n, 0), kt], 2).contiguous()
    vc = torch.cat([vp.repeat_interleave(n, 0), vt], 2).contiguous()
    kmc = torch.ones(B, Lp + Lt, dtype=torch.int32, device=dev)
    q, o = torch.randn(B, Hq, device=dev).to(bf), torch.empty(B, Hq, dtype=bf, device=dev)
    l = _hip.lib()
    ws = torch.empty(int(l.vlr_attn_decode_shared_workspace_bytes(P, n, nh, Lp, Lt)), dtype=torch.uint8, device=dev)
    wg = torch.empty(int(l.vlr_attn_decode_workspace_bytes(B, nh, Lp + Lt)), dtype=torch.uint8, device=dev)
    kv = _hip.KvShared(kp.data_ptr(), vp.data_ptr(), km.data_ptr(), P, Lp, Lp, kt.data_ptr(), vt.data_ptr(), n, Lt, Lt)
    sc = 1.0 / math.sqrt(hd)
    t = dict(shared=[], gqa=[])
    for _ in range(reps):
        s = ev()
        _hip.call("vlr_attn_decode_shared", q, Hq, kv, o, Hq, ws, nh, nkv, hd, sc)
        m = ev()
        _hip.call("vlr_attn_decode_gqa", q, Hq, kc, vc, kmc, o, Hq, wg, B, nh, nkv, hd, Lp + Lt, Lp + Lt, sc)
        e = ev()
        torch.cuda.synchronize()
        t["shared"].append(s.elapsed_time(m))
        t["gqa"].append(m.elapsed_time(e))
    return dict(shared_ms=stats(t["shared"]), gqa_materialised_ms=stats(t["gqa"]),
                shared_kv_bytes_one_layer=2 * 2 * nkv * hd * (P * Lp + B * Lt), materialised_kv_bytes_one_layer=2 * 2 * nkv * hd * B * (Lp + Lt))


def llava7b(a):
    import torch
    from vlrlhf.models.Llava import LlavaForRL
    from vlrlhf.utils.synthetic import LLAVA_1_5_7B, init_random_model, synthetic_batch
    cfg = dict(LLAVA_1_5_7B, layers=a.layers)
    model = LlavaForRL(cfg)
    eng = model.engine
    init_random_model(model, seed=0, std=0.02)
    model.eval()
    P = 4
    batch = synthetic_batch(P, 1024, cfg["image_token"], 32000, cfg["image_size"], seed=1234, prompt_frac=1.0)
    ids, mask = batch["prompt_input_ids"].to(eng.dev), batch["prompt_attention_mask"].to(eng.dev)
    pv = batch["img_input_dict"]["pixel_values"].to(eng.dev)
    ws = eng.policy
    out = []
    with torch.no_grad():
        for n in a.fanouts:
            ids_r, mask_r, pv_r = ids.repeat_interleave(n, 0), mask.repeat_interleave(n, 0), pv.repeat_interleave(n, 0)
            pre = dict(shared=[], repeated=[])
            for _ in range(3):                   # the prefills alternate too; the first pair is warm-up
                shared = eng.new_shared_kv_cache(P, n, a.new + 1)
                s = ev()
                c = eng.forward_hidden(ws, ids, mask, None, pv, save=False, tag="policy_ng", kv_cache=shared.prompt)
                tok_s = model._last_logits(c, P, ws.v["lm_head"]).argmax(-1).repeat_interleave(n)
                m = ev()
                rep = eng.new_kv_cache(P * n, a.new + 1)
                c = eng.forward_hidden(ws, ids_r, mask_r, None, pv_r, save=False, tag="policy_ng", kv_cache=rep)
                tok_r = model._last_logits(c, P * n, ws.v["lm_head"]).argmax(-1)
                e = ev()
                torch.cuda.synchronize()
                pre["shared"].append(s.elapsed_time(m))
                pre["repeated"].append(m.elapsed_time(e))
            S = c["S"]
            shared.begin()
            t = dict(shared=[], repeated=[])
            for _ in range(a.new):
                s = ev()
                tok_s = eng.decode_step(ws, tok_s, shared).argmax(-1)
                m = ev()
                tok_r = eng.decode_step(ws, tok_r, rep).argmax(-1)
                e = ev()
                torch.cuda.synchronize()
                t["shared"].append(s.elapsed_time(m))
                t["repeated"].append(m.elapsed_time(e))
            sh, rp = stats(t["shared"]), stats(t["repeated"])
            out.append(dict(fanout=n, prompts=P, merged_rows=S, layers=eng.L,
                            prefill_ms=dict(shared=round(min(pre["shared"][1:]), 1), repeated=round(min(pre["repeated"][1:]), 1)),
                            ms_per_token=dict(shared=sh, repeated=rp, shared_over_repeated=round(sh["median"] / rp["median"], 3)),
                            kv_bytes=dict(shared=shared.nbytes(), repeated=2 * rep.k.numel() * rep.k.element_size()),
                            attention_alone=attn_alone(P, n, eng.nh, eng.nkv, S, a.new + 1)))
            del shared, rep
            torch.cuda.empty_cache()
    return dict(llava7b=out)


def mistral(a):
    return dict(mistral_attention_2x4975=[dict(fanout=n, **attn_alone(2, n, 32, 8, 4975, a.new + 1)) for n in a.fanouts])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", choices=["", "llava7b", "mistral"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_shared_prompt.txt"))
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--new", type=int, default=40)
    ap.add_argument("--fanouts", default="2,4,8")
    ap.add_argument("--errors", default="")
    a = ap.parse_args()
    if a.only:                                   # one measurement, in this process
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("decode_shared_bench.py measures on the MI355X: no GPU here")
        a.fanouts = [int(x) for x in a.fanouts.split(",")]
        res = dict(llava7b=llava7b, mistral=mistral)[a.only](a)
        res["device"] = torch.cuda.get_device_name(0)
        print("RESULT " + json.dumps(res))
        return
    lines = []
    for name in ("mistral", "llava7b"):          # chained: a failure (or a time limit) ends the run, nothing else is started
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--only", name, "--layers", str(a.layers),
               "--new", str(a.new), "--fanouts", a.fanouts]
        r = subprocess.run(cmd, capture_output=True, text=True)
        res = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"decode_shared_bench.py: {name} failed with status {r.returncode}; stopping")
        lines.append(json.dumps(json.loads(res[-1][len("RESULT "):]), indent=1))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# tools/decode_shared_bench.py: n samples per prompt - the shared prompt cache against the prompts repeated n times in the batch\n"
                "# (ms: HIP events, medians with min .. max after 8 warm-up steps, the two routes alternating in one process)\n" + "\n".join(lines) + "\n")
        if a.errors and os.path.exists(a.errors):
            f.write("# errors the GPU tests measured (worst case per test)\n" + open(a.errors).read())


if __name__ == "__main__":
    main()
