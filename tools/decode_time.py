#!/usr/bin/env python3
"""KV-cache decoding on the MI355X: prefill time, decode time per new token, the re-forward loop (use_cache=False) per token, and the
bandwidth the decode step and its kernels reach.

    python tools/decode_time.py [--model llava|llava_next] [--prompts 4] [--text-len 1024] [--new 128] [--nocache-steps 3]
                                [--kernels] [--out FILE.json]

Set-up: synthetic LLaVA-1.5-7B (utils/synthetic init_hashed_model, synthetic_batch with prompt_frac 1.0: 4 prompts of 1024 text tokens
+ one 336^2 image = 1599 merged rows) or LLaVA-Next-Mistral-7B (2 prompts of 2048 tokens + a 672^2 anyres image), greedy decoding.
Times are HIP events on the launch stream; decode per token = median over the steps after the first 8 (warm-up).  Achieved
bandwidth of a decode step = (decoder + lm-head weight bytes + the K / V bytes the step reads) / step time, against 6.3 TB/s (the
float4 copy rate of MI355X_MICROARCH.md).  --kernels: the skinny GEMM at the 7B projection shapes and the decode attention alone
(event-timed, weights cycled through copies totalling >= 1 GiB so that no call reads from the 256 MiB Infinity Cache).
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vl-rlhf_amd"))
sys.path.insert(0, ROOT)

COPY_TBS = 6.3


def ev():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def model_and_prompts(a):
    from vlrlhf.utils.synthetic import LLAVA_1_5_7B, init_hashed_model, synthetic_batch
    if a.model == "llava_next":
        from vlrlhf.models.LlavaNext import LLAVA_NEXT_MISTRAL_7B, LlavaNextForRL as Cls
        from vlrlhf.utils.synthetic import synthetic_batch_anyres
        cfg = dict(LLAVA_NEXT_MISTRAL_7B)
        batch = synthetic_batch_anyres(a.prompts, a.text_len, cfg["image_token"], 32000, cfg["image_size"], seed=1234, prompt_frac=1.0)
    else:
        from vlrlhf.models.Llava import LlavaForRL as Cls
        cfg = dict(LLAVA_1_5_7B)
        batch = synthetic_batch(a.prompts, a.text_len, cfg["image_token"], 32000, cfg["image_size"], seed=1234, prompt_frac=1.0)
    if a.layers:
        cfg["layers"] = a.layers
    model = Cls(cfg)
    init_hashed_model(model, seed=0, std=0.02, policy_delta=1e-3)
    model.eval()
    dev = model.engine.dev
    kw = dict(input_ids=batch["prompt_input_ids"].to(dev), attention_mask=batch["prompt_attention_mask"].to(dev),
              **{k: v.to(dev) for k, v in batch["img_input_dict"].items()})
    return model, kw


def weight_bytes(e):
    per_layer = (e.Nqkv * e.H + e.H * e.Nq + 2 * e.I * e.H + e.H * e.I) * 2 + 2 * e.H * 2
    return e.L * per_layer + e.V * e.H * 2 + e.H * 2


def cached_run(model, kw, new):
    """prefill + `new` - 1 decode steps, timed; -> (prefill ms, [decode ms], tokens, cache)"""
    eng = model.engine
    ids = kw["input_ids"]
    B, T = ids.shape
    Tp = (T + 31) // 32 * 32
    if Tp != T:
        fill = torch.zeros(B, Tp - T, dtype=ids.dtype, device=ids.device)
        ids, mask = torch.cat([fill, ids], 1), torch.cat([torch.zeros_like(fill), kw["attention_mask"]], 1)
    else:
        mask = kw["attention_mask"]
    pv = kw["pixel_values"]
    with torch.no_grad():
        torch.cuda.synchronize()
        s = ev()
        cache = eng.new_kv_cache(B, new)
        c = eng.forward_hidden(model.weights, ids, mask, None, pv, save=False, tag="policy_ng", image_sizes=kw.get("image_sizes"), kv_cache=cache)
        logits = model._last_logits(c, B, model.weights.v["lm_head"])
        e = ev()
        toks = [logits.argmax(-1)]
        steps = []
        for _ in range(new - 1):
            s1 = ev()
            logits = eng.decode_step(model.weights, toks[-1], cache)
            e1 = ev()
            steps.append((s1, e1))
            toks.append(logits.argmax(-1))
        torch.cuda.synchronize()
    return s.elapsed_time(e), [x.elapsed_time(y) for x, y in steps], torch.stack(toks, 1), cache, c["S"]


def kernels(eng):
    """skinny GEMM at the decoder / lm-head shapes (M = 4) and decode attention at the bench cache, event-timed"""
    from vlrlhf import _hip
    out = {}
    M = 4
    shapes = dict(qkv=(eng.Nqkv, eng.H), o_proj=(eng.H, eng.Nq), gate_up=(2 * eng.I, eng.H), down=(eng.H, eng.I), lm_head=(eng.V, eng.H))
    modes = dict(qkv=_hip.GEMV_BF16, o_proj=_hip.GEMV_F32RES, gate_up=_hip.GEMV_SWIGLU, down=_hip.GEMV_F32RES, lm_head=_hip.GEMV_F32)
    X16 = torch.randn(M, 16384, device=eng.dev).bfloat16()
    for name, (N, K) in shapes.items():
        nbytes = N * K * 2
        copies = max(2, -(-(1 << 30) // nbytes))
        Ws = [torch.randn(N, K, device=eng.dev).bfloat16() * 0.02 for _ in range(copies)]
        ncols = N // 2 if modes[name] == _hip.GEMV_SWIGLU else N
        Y = torch.zeros(M, ncols, dtype=torch.float32 if modes[name] in (_hip.GEMV_F32, _hip.GEMV_F32RES) else torch.bfloat16, device=eng.dev)
        ws = torch.empty(int(_hip.lib().vlr_gemv_workspace_bytes(M, N, K)), dtype=torch.uint8, device=eng.dev)
        X = X16[:, :K].contiguous()
        res = Y if modes[name] == _hip.GEMV_F32RES else None

        def call(W):
            _hip.call("vlr_gemv_bf16", modes[name], X, K, W, Y, ncols, None, res, ncols if res is not None else 0, None, None, None, 0, 128,
                      0, M, N, K, ws)
        for W in Ws[:2]:
            call(W)
        reps = 3 * copies
        torch.cuda.synchronize()
        s = ev()
        for i in range(reps):
            call(Ws[i % copies])
        e = ev()
        torch.cuda.synchronize()
        us = s.elapsed_time(e) * 1e3 / reps
        out[name] = dict(N=N, K=K, M=M, us=round(us, 2), weight_TBs=round(nbytes / us / 1e6, 3), frac_of_copy=round(nbytes / us / 1e6 / COPY_TBS, 3))
        del Ws
    # decode attention at the bench cache (4 sequences x 1599 + 64 columns, all heads)
    B, L = 4, 1663
    nh, nkv, hd = eng.nh, eng.nkv, eng.hd
    kvb = B * nkv * L * hd * 2 * 2
    copies = max(2, -(-(1 << 30) // kvb))
    caches = [(torch.randn(B, nkv, L, hd, device=eng.dev).bfloat16(), torch.randn(B, nkv, L, hd, device=eng.dev).bfloat16()) for _ in range(copies)]
    q = torch.randn(B, eng.Nqkv, device=eng.dev).bfloat16()
    km = torch.ones(B, L, dtype=torch.int32, device=eng.dev)
    o = torch.empty(B, eng.Nq, dtype=torch.bfloat16, device=eng.dev)
    ws = torch.empty(int(_hip.lib().vlr_attn_decode_workspace_bytes(B, nh, L)), dtype=torch.uint8, device=eng.dev)

    def att(kv):
        _hip.call("vlr_attn_decode_gqa", q, eng.Nqkv, kv[0], kv[1], km, o, eng.Nq, ws, B, nh, nkv, hd, L, L, 1.0 / hd ** 0.5)
    att(caches[0])
    reps = 3 * copies
    torch.cuda.synchronize()
    s = ev()
    for i in range(reps):
        att(caches[i % copies])
    e = ev()
    torch.cuda.synchronize()
    us = s.elapsed_time(e) * 1e3 / reps
    out["attn_decode"] = dict(B=B, len=L, heads=nh, kv_heads=nkv, us=round(us, 2), kv_TBs=round(kvb / us / 1e6, 3),
                              frac_of_copy=round(kvb / us / 1e6 / COPY_TBS, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llava", choices=["llava", "llava_next"])
    ap.add_argument("--prompts", type=int, default=None)
    ap.add_argument("--text-len", type=int, default=None)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--nocache-steps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.prompts is None:
        a.prompts = 2 if a.model == "llava_next" else 4
    if a.text_len is None:
        a.text_len = 2048 if a.model == "llava_next" else 1024
    if not torch.cuda.is_available():
        raise SystemExit("decode_time.py measures on the MI355X: no GPU here")
    model, kw = model_and_prompts(a)
    eng = model.engine
    cached_run(model, kw, 12)                                          # warm-up: code objects, vision cache, workspaces
    pre_ms, steps, toks, cache, S = cached_run(model, kw, a.new)
    warm = steps[8:] if len(steps) > 16 else steps
    dec_ms = statistics.median(warm)
    B = kw["input_ids"].shape[0]
    wb = weight_bytes(eng)
    kv_mean = eng.L * B * eng.nkv * (S + a.new / 2) * eng.hd * 2 * 2
    res = dict(model=a.model, prompts=B, text_len=a.text_len, merged_rows=S, new_tokens=a.new, layers=eng.L,
               prefill_ms=round(pre_ms, 2), decode_ms_per_token=round(dec_ms, 3),
               decode_ms_min=round(min(warm), 3), decode_ms_max=round(max(warm), 3),
               step_weight_GB=round(wb / 1e9, 3), step_kv_GB_mean=round(kv_mean / 1e9, 3),
               achieved_TBs=round((wb + kv_mean) / dec_ms / 1e9, 3))
    res["frac_of_copy"] = round(res["achieved_TBs"] / COPY_TBS, 3)
    if a.nocache_steps > 0:
        with torch.no_grad():
            g = dict(kw, max_new_tokens=1, do_sample=False, pad_token_id=0, eos_token_id=10 ** 6, use_cache=False)
            model.generate(**g)                                        # warm-up
            torch.cuda.synchronize()
            s = ev()
            ref = model.generate(**dict(g, max_new_tokens=a.nocache_steps))
            e = ev()
            torch.cuda.synchronize()
        res["nocache_ms_per_token"] = round(s.elapsed_time(e) / a.nocache_steps, 2)
        res["speedup_per_token"] = round(res["nocache_ms_per_token"] / dec_ms, 1)
        T = kw["input_ids"].shape[1]
        res["greedy_tokens_agree_with_nocache"] = int(sum(bool(torch.equal(ref[:, T + k], toks[:, k])) for k in range(a.nocache_steps)))
    if a.kernels:
        res["kernels"] = kernels(eng)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
