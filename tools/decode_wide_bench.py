#!/usr/bin/env python3
"""The wide skinny GEMM (vlr_gemv_wide_bf16: up to 64 rows per pass over the weights) and Qwen-VL's KV cache on the MI355X, measured.

    python tools/decode_wide_bench.py [--out profiles/decode_wide.txt] [--layers 32] [--new 24]

Two measurements, each in a process of its own under its own time limit; the driver stops at the first one that fails:
  kernels  (a) the five 7B shapes of tests/test_hip_decode_kernels.py SHAPES_7B and the Qwen-VL lm-head (K 4096, N 151936) at M = 17, 32,
           48, 64 rows: one vlr_gemv_wide_bf16 call against the same rows through vlr_gemv_bf16 in 16-row groups (what the layer driver
           did before the wide path, and still does without wide scratch).  The two sides alternate in blocks inside one process; the
           weights are cycled through >= 1 GiB of copies so that no call reads them from the Infinity Cache.  Next to them: a device copy
           of one weight matrix.  Rates are weight bytes (N K 2) over the call time - for the copy, the bytes copied over its time.
  tokens   (b) Qwen-VL-Chat widths, LoRA r 64 (live adapters: how PPO samples), 32 prompts of one image + 64 text tokens: ms per new
           token of the re-forward loop, of the cached route with 16-row groups (engine.wide_gemv = False: the wide scratch withheld)
           and of the cached route with the wide GEMMs, the two cached routes in alternating blocks of steps.
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

LIMITS = dict(kernels=300, tokens=560)                                       # seconds per measurement
SHAPES = [("qkv", 4096, 12288), ("o_proj", 4096, 4096), ("gate|up", 4096, 22016), ("down", 11008, 4096), ("lm-head 32000", 4096, 32000),
          ("lm-head Qwen-VL", 4096, 151936)]                                 # (name, K, N)
ROWS = (17, 32, 48, 64)


def ev():
    import torch
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def kernels(a):
    import torch
    from vlrlhf import _hip
    lib, dev = _hip.lib(), "cuda"
    out = []
    for name, K, N in SHAPES:
        copies = max(2, -(-(1 << 30) // (N * K * 2)))
        W = [(torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16) for _ in range(copies)]
        X = torch.randn(64, K, device=dev).to(torch.bfloat16)
        Yw, Yg = (torch.empty(64, N, dtype=torch.float32, device=dev) for _ in range(2))
        ws = torch.empty(int(lib.vlr_gemv_wide_workspace_bytes(64, N, K)), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(W[0])
        reps = max(2 * copies, 64)                       # a timed block is 64 or more calls

        def wide(M, i):
            _hip.call("vlr_gemv_wide_bf16", _hip.GEMV_F32, X, K, W[i % copies], Yw, N, None, None, 0, None, None, None, 0, 128, 4096, M, N, K, ws)

        def groups(M, i):
            for m0 in range(0, M, 16):
                _hip.call("vlr_gemv_bf16", _hip.GEMV_F32, X[m0:], K, W[i % copies], Yg[m0:], N, None, None, 0, None, None, None, 0, 128, 4096,
                          min(16, M - m0), N, K, ws)

        def block(fn, M):
            s = ev()
            for i in range(reps):
                fn(M, i)
            e = ev()
            torch.cuda.synchronize()
            return s.elapsed_time(e) * 1e3 / reps

        s = ev()
        for i in range(reps):
            dst.copy_(W[i % copies])
        e = ev()
        torch.cuda.synchronize()                         # (warm-up of the copy)
        t_copy = []
        row = dict(shape=name, K=K, N=N, weight_MB=round(N * K * 2 / 1e6, 1), rows={})
        for M in ROWS:
            wide(M, 0)
            groups(M, 0)
            torch.cuda.synchronize()
            assert torch.equal(Yw[:M], Yg[:M]), (name, M)            # faster and different is not faster
            tw, tg = [], []
            for _ in range(a.rounds):                    # the sides alternate: same clocks, same neighbours
                tw.append(block(wide, M))
                tg.append(block(groups, M))
                s = ev()
                for i in range(reps):
                    dst.copy_(W[i % copies])
                e = ev()
                torch.cuda.synchronize()
                t_copy.append(s.elapsed_time(e) * 1e3 / reps)
            w, g = statistics.median(tw), statistics.median(tg)
            row["rows"][M] = dict(wide_us=round(w, 1), groups_us=round(g, 1), wide_TBps=round(N * K * 2 / w / 1e6, 2),
                                  groups_TBps=round(N * K * 2 / g / 1e6, 2), groups_over_wide=round(g / w, 2))
        c = statistics.median(t_copy)
        row["copy_us"], row["copy_TBps"] = round(c, 1), round(N * K * 2 / c / 1e6, 2)
        out.append(row)
        del W, dst, Yw, Yg
        torch.cuda.empty_cache()
    return dict(kernels=out)


def tokens(a):
    import torch
    from vlrlhf.models.QwenVL import QWEN_VL_CHAT, QwenVLForRL
    from vlrlhf.utils.synthetic import init_hashed_qwen
    cfg = dict(QWEN_VL_CHAT, layers=a.layers)
    model = QwenVLForRL(cfg)
    eng = model.engine
    init_hashed_qwen(model, seed=0, std=0.02, with_reference=False)
    model.apply_lora(dict(r=64, lora_alpha=16, lora_dropout=0.05, target_modules="auto", bias="none"))
    g = torch.Generator(device=eng.dev).manual_seed(5)
    for v in eng.lv.values():
        v.copy_((torch.randn(v.shape, generator=g, device=eng.dev) * 0.01).to(v.dtype))
    model.eval()
    model.enable_kv_cache()
    B, st, nq, size = 32, cfg["image_start_id"], cfg["visual"].get("n_queries", 256), cfg["visual"]["image_size"]
    gc = torch.Generator().manual_seed(1234)
    rows = []
    for i in range(B):                                   # one image (<img> + 256 slots + </img>) and 64 text tokens
        path = list(f"synthetic/{i}.png".encode())
        text = torch.randint(256, st - 1, (64,), generator=gc).tolist()
        rows.append(text[:3] + [st] + path + [st + 2] * (nq - len(path)) + [st + 1] + text[3:])
    ids = torch.tensor(rows, dtype=torch.long, device=eng.dev)
    mask = torch.ones_like(ids)
    pv = torch.randn(B, 3, size, size, generator=gc).to(eng.dev)
    kw = dict(input_ids=ids, attention_mask=mask, pixel_values=pv, do_sample=False, pad_token_id=cfg.get("pad_token_id", 0), eos_token_id=10 ** 9,
              use_cache=False, merge_lora=False)
    blocks, per = 4, a.new
    t = dict(wide=[], groups=[], reforward=[])
    with torch.no_grad():
        caches, toks = {}, {}
        for key in ("wide", "groups"):
            cache = eng.new_kv_cache(B, blocks * per // 2 + 1)
            c = eng.forward_hidden(eng.policy, ids, mask, None, pv, save=False, tag="policy_ng", kv_cache=cache)
            caches[key], toks[key] = cache, model._last_logits(c, B, eng.policy.v["lm_head"]).argmax(-1).clamp(max=st - 1)
        for b in range(blocks):                          # wide, groups, wide, groups: blocks of steps, the first 4 of a block dropped
            key = ("wide", "groups")[b % 2]
            eng.wide_gemv = key == "wide"
            for i in range(per):
                s = ev()
                logits = eng.decode_step(eng.policy, toks[key], caches[key])
                e = ev()
                torch.cuda.synchronize()
                toks[key] = logits.argmax(-1).clamp(max=st - 1)
                if i >= 4:
                    t[key].append(s.elapsed_time(e))
        eng.wide_gemv = True
        for _ in range(3):                               # the re-forward loop: two tokens minus one (vision features cached in both)
            s = ev()
            model.generate(max_new_tokens=1, **kw)
            m = ev()
            model.generate(max_new_tokens=2, **kw)
            e = ev()
            torch.cuda.synchronize()
            t["reforward"].append(m.elapsed_time(e) - s.elapsed_time(m))
    med = {k: statistics.median(v) for k, v in t.items()}
    return dict(tokens=dict(layers=eng.L, rank=64, rows=B, prompt_columns=int(ids.shape[1]), steps_timed={k: len(v) for k, v in t.items()},
                            reforward_ms_per_token=round(med["reforward"], 2), cached_16_row_groups_ms_per_token=round(med["groups"], 3),
                            cached_wide_ms_per_token=round(med["wide"], 3),
                            spread_wide_ms=[round(min(t["wide"]), 3), round(max(t["wide"]), 3)],
                            spread_groups_ms=[round(min(t["groups"]), 3), round(max(t["groups"]), 3)],
                            groups_over_wide=round(med["groups"] / med["wide"], 3), reforward_over_wide=round(med["reforward"] / med["wide"], 1)))


def render(res):
    L = ["The wide skinny GEMM and Qwen-VL on the KV cache, one MI355X (tools/decode_wide_bench.py; random weights, HIP events, medians)", ""]
    if "kernels" in res:
        L += ["(a) one vlr_gemv_wide_bf16 call against the same rows through vlr_gemv_bf16 in 16-row groups (fp32 out, no bias), alternating blocks;",
              "    weights cycled through >= 1 GiB of copies; TB/s = weight bytes (N K 2) / call time; copy = torch copy_ of one weight matrix,",
              "    its rate = bytes copied / time.  Outputs compared bit for bit before timing.", "",
              f"  {'shape':<16}{'N x K':<16}{'M':>4}{'wide us':>10}{'groups us':>11}{'groups/wide':>13}{'wide TB/s':>11}{'groups TB/s':>13}{'copy us':>9}{'copy TB/s':>11}"]
        for r in res["kernels"]:
            for M, v in r["rows"].items():
                L.append(f"  {r['shape']:<16}{str(r['N']) + ' x ' + str(r['K']):<16}{M:>4}{v['wide_us']:>10}{v['groups_us']:>11}{v['groups_over_wide']:>13}"
                         f"{v['wide_TBps']:>11}{v['groups_TBps']:>13}{r['copy_us']:>9}{r['copy_TBps']:>11}")
        slower = [f"{r['shape']} M {M}" for r in res["kernels"] for M, v in r["rows"].items() if v["groups_over_wide"] < 1.0]
        L += ["", "  dispatch rule (csrc/layers.cpp gemv_rows, engine._gemv_rows): batch > 16 over bf16 weights with wide scratch -> 64-row groups "
              "through the wide call;", "  the wide call is slower than the 16-row groups at: " + (", ".join(slower) if slower else "no shape and no M measured here")
              + (" - REVISIT the rule for these" if slower else " - the rule has no exception"), ""]
    if "tokens" in res:
        t = res["tokens"]
        L += [f"(b) Qwen-VL-Chat widths, {t['layers']} layers, LoRA r {t['rank']} live (merge_lora=False), {t['rows']} prompts of {t['prompt_columns']} columns "
              "(one image + 64 text tokens), ms per new token:", "",
              f"  re-forward loop (a fresh model; generate of 2 tokens minus generate of 1)   {t['reforward_ms_per_token']}",
              f"  KV cache, 16-row groups (wide scratch withheld)                            {t['cached_16_row_groups_ms_per_token']}   "
              f"({t['spread_groups_ms'][0]} - {t['spread_groups_ms'][1]})",
              f"  KV cache, wide GEMMs                                                       {t['cached_wide_ms_per_token']}   "
              f"({t['spread_wide_ms'][0]} - {t['spread_wide_ms'][1]})",
              f"  groups / wide {t['groups_over_wide']}; re-forward / wide {t['reforward_over_wide']}; steps timed {t['steps_timed']}", ""]
    L.append("device: " + res.get("device", "?"))
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", choices=["", "kernels", "tokens"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_wide.txt"))
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--new", type=int, default=24, help="decode steps per block (4 blocks: wide, groups, wide, groups)")
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the two sides per kernel shape and M")
    a = ap.parse_args()
    if a.only:                                   # one measurement, in this process
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("decode_wide_bench.py measures on the MI355X: no GPU here")
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
            raise SystemExit(f"decode_wide_bench.py: {name} failed with status {r.returncode}; stopping")
        res.update(json.loads(got[-1][len("RESULT "):]))
        print(got[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(render(res))
    print(render(res))


if __name__ == "__main__":
    main()
