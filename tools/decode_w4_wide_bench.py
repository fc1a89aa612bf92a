#!/usr/bin/env python3
"""The wide skinny GEMM over packed int4 weights (vlr_gemv_wide_w4: up to 64 rows per pass over the packed words) on the MI355X, measured.

    python tools/decode_w4_wide_bench.py [--out profiles/decode_w4_wide.txt] [--layers 32] [--new 24]

Two measurements, each in a process of its own under its own time limit; the driver stops at the first one that fails:
  kernels  (a) the four decoder projection shapes of LLaVA-1.5-7B, GPTQ group 128, at M = 17, 32, 48, 64 rows: one vlr_gemv_wide_w4 call
           against the same rows through vlr_gemv_w4 in 16-row groups (what the layer driver did before the wide path, and still does
           without wide scratch).  The two sides alternate in blocks inside one process; the packed weights are cycled through >= 1 GiB
           of copies so that no call reads them from the Infinity Cache.  Rates are packed bytes (qweight + scales + qzeros) over the
           call time.
  tokens   (b) a packed LLaVA-1.5-7B (q_lora base, no adapters), 32 prompts of one image + 64 text tokens: ms per new token of the cached
           route with 16-row groups (engine.wide_gemv = False: the wide scratch withheld) and with the wide GEMMs, in alternating blocks
           of steps.
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

LIMITS = dict(kernels=300, tokens=400)                                       # seconds per measurement
SHAPES = [("qkv", 4096, 12288), ("o_proj", 4096, 4096), ("gate|up", 4096, 22016), ("down", 11008, 4096)]      # (name, K, N)
ROWS = (17, 32, 48, 64)
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
    lib, dev = _hip.lib(), "cuda"
    out = []
    for name, K, N in SHAPES:
        packed_bytes = N * K // 2 + (K // G) * N * 2 + (K // G) * N // 2
        copies = max(2, -(-(1 << 30) // packed_bytes))
        Q = [random_packed(K, N, G, dev) for _ in range(copies)]
        X = torch.randn(64, K, device=dev).to(torch.bfloat16)
        Yw, Yg = (torch.empty(64, N, dtype=torch.float32, device=dev) for _ in range(2))
        ws = torch.empty(int(lib.vlr_gemv_wide_w4_workspace_bytes(64, N, K)), dtype=torch.uint8, device=dev)
        reps = max(copies, 64)                           # a timed block is 64 or more calls

        def wide(M, i):
            _hip.call("vlr_gemv_wide_w4", _hip.GEMV_F32, X, K, *Q[i % copies], G, Yw, N, None, None, 0, None, None, None, 0, 128, 4096, M, N, K, ws)

        def groups(M, i):
            for m0 in range(0, M, 16):
                _hip.call("vlr_gemv_w4", _hip.GEMV_F32, X[m0:], K, *Q[i % copies], G, Yg[m0:], N, None, None, 0, None, None, None, 0, 128, 4096,
                          min(16, M - m0), N, K, ws)

        def block(fn, M):
            s = ev()
            for i in range(reps):
                fn(M, i)
            e = ev()
            torch.cuda.synchronize()
            return s.elapsed_time(e) * 1e3 / reps

        row = dict(shape=name, K=K, N=N, packed_MB=round(packed_bytes / 1e6, 1), rows={})
        for M in ROWS:
            wide(M, 0)
            groups(M, 0)
            torch.cuda.synchronize()
            assert torch.equal(Yw[:M], Yg[:M]), (name, M)            # faster and different is not faster
            block(wide, M), block(groups, M)                         # warm
            tw, tg = [], []
            for _ in range(a.rounds):                    # the sides alternate: same clocks, same neighbours
                tw.append(block(wide, M))
                tg.append(block(groups, M))
            w, g = statistics.median(tw), statistics.median(tg)
            row["rows"][M] = dict(wide_us=round(w, 1), groups_us=round(g, 1), wide_TBps=round(packed_bytes / w / 1e6, 2),
                                  groups_TBps=round(packed_bytes * -(-M // 16) / g / 1e6, 2), groups_over_wide=round(g / w, 2),
                                  wide_spread_us=[round(min(tw), 1), round(max(tw), 1)], groups_spread_us=[round(min(tg), 1), round(max(tg), 1)])
        out.append(row)
        del Q, Yw, Yg
        torch.cuda.empty_cache()
    return dict(kernels=out)


def tokens(a):
    import torch
    from vlrlhf import gptq
    from vlrlhf.models.Llava import LlavaForRL
    from vlrlhf.utils.synthetic import LLAVA_1_5_7B, init_random_model, synthetic_batch
    cfg = dict(LLAVA_1_5_7B, layers=a.layers, gptq=dict(bits=4, group_size=G))
    model = LlavaForRL(cfg)
    eng = model.engine
    for name, shape, _ in eng.layout.entries:
        if name in eng.layout.packed:
            eng.packed[name] = gptq.PackedLinear(*random_packed(shape[1], shape[0], G, eng.dev), G)
    init_random_model(model, seed=0, std=0.02)
    model.eval()
    B = 32
    batch = synthetic_batch(B, 64, cfg["image_token"], 32000, cfg["image_size"], seed=1234, prompt_frac=1.0)
    ids, mask = batch["prompt_input_ids"].to(eng.dev), batch["prompt_attention_mask"].to(eng.dev)
    pv = batch["img_input_dict"]["pixel_values"].to(eng.dev)
    assert ids.shape[0] == B
    blocks, per = 4, a.new
    t = dict(wide=[], groups=[])
    with torch.no_grad():
        caches, toks = {}, {}
        for key in ("wide", "groups"):
            cache = eng.new_kv_cache(B, blocks * per // 2 + 1)
            c = eng.forward_hidden(model.weights, ids, mask, None, pv, save=False, tag="policy_ng", kv_cache=cache)
            caches[key], toks[key] = cache, model._last_logits(c, B, model.weights.v["lm_head"]).argmax(-1)
        for b in range(blocks):                          # wide, groups, wide, groups: blocks of steps, the first 4 of a block dropped
            key = ("wide", "groups")[b % 2]
            eng.wide_gemv = key == "wide"
            for i in range(per):
                s = ev()
                logits = eng.decode_step(model.weights, toks[key], caches[key])
                e = ev()
                torch.cuda.synchronize()
                toks[key] = logits.argmax(-1)
                if i >= 4:
                    t[key].append(s.elapsed_time(e))
        eng.wide_gemv = True
    med = {k: statistics.median(v) for k, v in t.items()}
    return dict(tokens=dict(layers=eng.L, rows=B, prompt_columns=int(c["S"]), group=G, steps_timed={k: len(v) for k, v in t.items()},
                            cached_16_row_groups_ms_per_token=round(med["groups"], 3), cached_wide_ms_per_token=round(med["wide"], 3),
                            spread_wide_ms=[round(min(t["wide"]), 3), round(max(t["wide"]), 3)],
                            spread_groups_ms=[round(min(t["groups"]), 3), round(max(t["groups"]), 3)],
                            groups_over_wide=round(med["groups"] / med["wide"], 3)))


def render(res):
    L = ["The wide skinny GEMM over packed int4 weights, one MI355X (tools/decode_w4_wide_bench.py; random weights, HIP events, medians)", ""]
    if "kernels" in res:
        L += [f"(a) one vlr_gemv_wide_w4 call against the same rows through vlr_gemv_w4 in 16-row groups (group {G}, fp32 out, no bias), alternating",
              "    blocks; packed weights cycled through >= 1 GiB of copies; TB/s = packed bytes read (qweight + scales + qzeros; the groups read",
              "    them ceil(M / 16) times) / call time; (min - max) over the alternations.  Outputs compared bit for bit before timing.", "",
              f"  {'shape':<10}{'N x K':<16}{'M':>4}{'wide us':>10}{'(min - max)':>18}{'groups us':>11}{'(min - max)':>18}{'groups/wide':>13}{'wide TB/s':>11}{'groups TB/s':>13}"]
        for r in res["kernels"]:
            for M, v in r["rows"].items():
                sw, sg = (f"({v[k][0]} - {v[k][1]})" for k in ("wide_spread_us", "groups_spread_us"))
                L.append(f"  {r['shape']:<10}{str(r['N']) + ' x ' + str(r['K']):<16}{M:>4}{v['wide_us']:>10}{sw:>18}{v['groups_us']:>11}{sg:>18}"
                         f"{v['groups_over_wide']:>13}{v['wide_TBps']:>11}{v['groups_TBps']:>13}")
        slower = [f"{r['shape']} M {M}" for r in res["kernels"] for M, v in r["rows"].items() if v["groups_over_wide"] < 1.0]
        L += ["", "  dispatch rule (csrc/layers.cpp gemv_rows): batch > 16 with wide scratch -> 64-row groups through the wide call, packed or bf16;",
              "  the wide packed call is slower than the 16-row groups at: " + (", ".join(slower) if slower else "no shape and no M measured here")
              + (" - REVISIT the rule for these" if slower else " - the rule has no exception"), ""]
    if "tokens" in res:
        t = res["tokens"]
        L += [f"(b) LLaVA-1.5-7B widths, {t['layers']} layers, decoder projections packed (group {t['group']}), no adapters, {t['rows']} prompts of "
              f"{t['prompt_columns']} merged columns (one image + 64 text tokens), ms per new token:", "",
              f"  KV cache, 16-row groups (wide scratch withheld)   {t['cached_16_row_groups_ms_per_token']}   ({t['spread_groups_ms'][0]} - {t['spread_groups_ms'][1]})",
              f"  KV cache, wide GEMMs                              {t['cached_wide_ms_per_token']}   ({t['spread_wide_ms'][0]} - {t['spread_wide_ms'][1]})",
              f"  groups / wide {t['groups_over_wide']}; steps timed {t['steps_timed']}", ""]
    L.append("device: " + res.get("device", "?"))
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", choices=["", "kernels", "tokens"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_w4_wide.txt"))
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--new", type=int, default=24, help="decode steps per block (4 blocks: wide, groups, wide, groups)")
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the two sides per kernel shape and M")
    a = ap.parse_args()
    if a.only:                                   # one measurement, in this process
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("decode_w4_wide_bench.py measures on the MI355X: no GPU here")
        res = dict(kernels=kernels, tokens=tokens)[a.only](a)
        res["device"] = torch.cuda.get_device_name(0)
        print("RESULT " + json.dumps(res))
        return
    res = {}
    for name in ("kernels", "tokens"):           # chained: a failure (or a time limit) ends the run, nothing else is started
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--only", name, "--layers", str(a.layers),
               "--new", str(a.new), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        got = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"decode_w4_wide_bench.py: {name} failed with status {r.returncode}; stopping")
        res.update(json.loads(got[-1][len("RESULT "):]))
        print(got[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(render(res))
    print(render(res))


if __name__ == "__main__":
    main()
