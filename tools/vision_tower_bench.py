#!/usr/bin/env python3
"""What the backward of a trainable CLIP-L tower costs at the headline batch (4 images x 577 tokens, 1024 wide, 16 heads of 64, MLP
4096, 23 evaluated layers), kernel level:

  * vlr_attn_bwd at head_dim 64, full attention (the call = attn_delta_kernel<64> + attn_bwd_dq_kernel<64> + attn_bwd_dkv_kernel<64>):
    ms per call and TF/s at 10 B heads S^2 D FLOPs, next to the forward;
  * vlr_vit_layer_fwd and vlr_vit_layer_bwd (recompute + backward) per layer, and x 23 layers: the ViT forward and backward per step;
  * vlr_vit_embed_ln_bwd + the patch kernel's weight-gradient GEMM;
  * the bytes the training pass keeps (every layer's input) and the backward's workspace.

Each figure is the mean of --reps calls between two HIP events, after a warm-up, in --blocks blocks; the block-to-block spread is
printed.

Then the step (--skip_step leaves it out): the LLaVA-1.5-7B headline configuration of bench.py (4 pairs, 1024 text tokens, S = 1599,
full fine-tune, the reference forward inside the step on the side stream, lr 2e-8) with the default frozen tower (A) and with the
tower trainable (B), in this process, interleaved A B A B.  One such engine peaks near 180 GiB, so each block builds its engine,
runs --step_warmup + --step_steps steps, reads torch.cuda.max_memory_allocated and frees everything before the next block builds.
In the B blocks HIP events bracket the policy's own ViT forward and engine._vision_backward in every timed step: their mean per step
over the step time is the tower's measured share (the reference forward may run beside them on the side stream).

    python tools/vision_tower_bench.py [--images 4] [--reps 20] [--blocks 2] [--skip_step] [--step_steps 4] [--step_layers N] [--out F]"""
import argparse
import gc
import time
from types import SimpleNamespace
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vl-rlhf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

KEYS = ("ln1_w", "ln1_b", "wqkv", "bqkv", "wo", "bo", "ln2_w", "ln2_b", "w1", "b1", "w2", "b2")


def step_block(train, a):
    """one block of the step-level A/B: build the engine, warm up, time a.step_steps steps, free it -> dict"""
    from vlrlhf.models.Llava import LlavaDPOTrainer, LlavaForRL
    from vlrlhf.utils.synthetic import LLAVA_1_5_7B, init_random_model, synthetic_batch
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    cfg = dict(LLAVA_1_5_7B)
    if a.step_layers:
        cfg["layers"] = a.step_layers
    if train:
        cfg["train_vision_tower"] = True
    model = LlavaForRL(cfg)
    ref = init_random_model(model, seed=0, std=0.02, policy_delta=1e-3)
    eng = model.engine
    tr = LlavaDPOTrainer(model, ref, 0.1, 0, "sigmoid", SimpleNamespace(gradient_accumulation_steps=1), None, -100, 0)
    eng.init_optimizer()
    tr.ref_on_side_stream = True
    batches = [tr._prepare_inputs(synthetic_batch(4, 1024, cfg["image_token"], 32000, cfg["image_size"], seed=1234 + 1000 * i)) for i in range(4)]
    hp = dict(lr=2e-8, beta1=0.9, beta2=0.98, eps=1e-6, weight_decay=0.0, max_grad_norm=1.0)
    ev = dict(fwd=[], bwd=[])

    def bracket(fn, key, when=lambda a_, k_: True):
        def wrapped(*a_, **k_):
            if not when(a_, k_):
                return fn(*a_, **k_)
            s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s_.record()
            out = fn(*a_, **k_)
            e_.record()
            ev[key].append((s_, e_))
            return out
        return wrapped

    if train:
        eng.vision_features = bracket(eng.vision_features, "fwd", lambda a_, k_: k_.get("keep") is not None)
        eng._vision_backward = bracket(eng._vision_backward, "bwd")
    n = [0]

    def step():
        loss = tr.training_step(model, batches[n[0] % 4])
        tr.prefetch_reference(batches[(n[0] + 1) % 4])
        eng.optimizer_step(grad_scale=1.0, **hp)
        n[0] += 1
        return loss

    for _ in range(a.step_warmup):
        step()
    torch.cuda.synchronize()
    ev["fwd"].clear(), ev["bwd"].clear()
    t0 = time.time()
    for _ in range(a.step_steps):
        loss = step()
    torch.cuda.synchronize()
    ms = (time.time() - t0) / a.step_steps * 1e3
    out = dict(train=train, ms=ms, loss=float(loss), peak_gib=torch.cuda.max_memory_allocated() / 2 ** 30, params=eng.layout.n_opt,
               vit_fwd_ms=sum(s_.elapsed_time(e_) for s_, e_ in ev["fwd"]) / a.step_steps,
               vit_bwd_ms=sum(s_.elapsed_time(e_) for s_, e_ in ev["bwd"]) / a.step_steps, calls=(len(ev["fwd"]), len(ev["bwd"])))
    ev["fwd"].clear(), ev["bwd"].clear()
    del model, ref, eng, tr, batches, step
    gc.collect()
    torch.cuda.empty_cache()
    return out


def step_ab(a):
    lines = [f"step: LLaVA-1.5-7B DPO, 4 pairs x 1024 text tokens (S = 1599), full fine-tune, "
             f"{'32' if not a.step_layers else a.step_layers} decoder layers, reference forward in the step; {a.step_warmup} warm-up + "
             f"{a.step_steps} timed steps per block, the engine rebuilt for every block, blocks interleaved A (frozen tower) B (trainable tower) A B"]
    res = []
    for i, train in enumerate((False, True, False, True)):
        r = step_block(train, a)
        res.append(r)
        extra = (f", policy ViT forward {r['vit_fwd_ms']:.2f} ms + ViT backward {r['vit_bwd_ms']:.2f} ms per step between HIP events "
                 f"({r['calls'][0]} + {r['calls'][1]} calls) = {100 * (r['vit_fwd_ms'] + r['vit_bwd_ms']) / r['ms']:.2f} % of the step "
                 f"(backward alone {100 * r['vit_bwd_ms'] / r['ms']:.2f} %)") if train else ""
        lines.append(f"block {i} {'B trainable' if train else 'A frozen   '}: {r['ms']:.2f} ms per step, peak allocated {r['peak_gib']:.1f} GiB, "
                     f"{r['params'] / 1e9:.3f} G trainable parameters, last loss {r['loss']:.5f}{extra}")
        print(lines[-1], flush=True)
    fa, tb = [r["ms"] for r in res if not r["train"]], [r["ms"] for r in res if r["train"]]
    ma, mb = sum(fa) / 2, sum(tb) / 2
    lines.append(f"frozen {ma:.2f} ms (blocks {fa[0]:.2f} / {fa[1]:.2f}, spread {abs(fa[0] - fa[1]):.2f}), trainable {mb:.2f} ms (blocks {tb[0]:.2f} / {tb[1]:.2f}, "
                 f"spread {abs(tb[0] - tb[1]):.2f}): +{mb - ma:.2f} ms = {100 * (mb / ma - 1):.2f} % per step; peak memory "
                 f"{max(r['peak_gib'] for r in res if not r['train']):.1f} -> {max(r['peak_gib'] for r in res if r['train']):.1f} GiB")
    lines.append("(the two layouts draw different random weights - the flat buffer the initialiser fills is longer with the tower in it - so the "
                 "losses of A and B differ; that the first step is the frozen step bit for bit is tests/test_hip_vision_tower_training.py's)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip_step", action="store_true", help="kernel level only")
    ap.add_argument("--step_steps", type=int, default=4)
    ap.add_argument("--step_warmup", type=int, default=1)
    ap.add_argument("--step_layers", type=int, default=None, help="fewer decoder layers than the model's 32 (said in the output)")
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--layers", type=int, default=23)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    from vlrlhf import _hip
    _hip.lib()
    _hip.ensure_splitk_workspace("cuda", force=True)
    dev, bf = "cuda", torch.bfloat16
    n, T, D, nh, F, Kp = a.images, 577, 1024, 16, 4096, 592
    M, Sp, hd = n * T, (T + 63) // 64 * 64, 64
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s, std=1.0: (torch.randn(*s, generator=g, device=dev) * std).to(bf)      # noqa: E731
    w = dict(ln1_w=1 + rn(D, std=0.1), ln1_b=rn(D, std=0.1), wqkv=rn(3 * D, D, std=D ** -0.5), bqkv=rn(3 * D, std=0.1), wo=rn(D, D, std=D ** -0.5),
             bo=rn(D, std=0.1), ln2_w=1 + rn(D, std=0.1), ln2_b=rn(D, std=0.1), w1=rn(F, D, std=D ** -0.5), b1=rn(F, std=0.1),
             w2=rn(D, F, std=F ** -0.5), b2=rn(D, std=0.1))
    gr = {k: torch.zeros_like(v) for k, v in w.items()}
    cfg = _hip.VitCfg(D, F, nh, hd, 1e-5, 1, 0, 0.0)
    ws_ = _hip.VitLayerWeights(*(w[k].data_ptr() for k in KEYS))
    gs_ = _hip.VitLayerGrads(*(gr[k].data_ptr() for k in KEYS))
    e = lambda *s, dt=bf: torch.empty(*s, dtype=dt, device=dev)      # noqa: E731
    fw = dict(xn=e(M, D), qkv=e(M, 3 * D), attn=e(M, D), h=e(M, F))
    fws = _hip.VitWs(*(fw[k].data_ptr() for k in ("xn", "qkv", "attn", "h")))
    nb = _hip.helper("vlr_vit_layer_bwd_workspace_bytes", D, F)
    b = dict(xn1=e(M, D), qkv=e(M, 3 * D), attn=e(M, D), lse=e(n, nh, Sp, dt=torch.float32), x_mid=e(M, D), xn2=e(M, D), z=e(M, F), h=e(M, F),
             dh=e(M, F), dxn=e(M, D), dqkv=e(M, 3 * D), delta=e(n, nh, Sp, dt=torch.float32), norm_ws=e(nb, dt=torch.uint8))
    b["dattn"] = b["dxn"]
    bws = _hip.VitBwdWs(*(b[k].data_ptr() for k, _ in _hip.VitBwdWs._fields_))
    x, dy = rn(M, D), rn(M, D)
    xw, dx = x.clone(), dy.clone()
    qkv, do, o, dqkv = rn(M, 3 * D), rn(M, D), e(M, D), e(M, 3 * D)
    lse, delta = e(n, nh, Sp, dt=torch.float32), e(n, nh, Sp, dt=torch.float32)
    scale = 1.0 / math.sqrt(hd)
    pe, cls, pos, dpe, patches = rn(n * (T - 1), D), rn(D), rn(T, D), e(n * (T - 1), D), rn(n * (T - 1), Kp)
    gcls, gpos, gw, gb, gpw = torch.zeros(D, dtype=bf, device=dev), torch.zeros(T, D, dtype=bf, device=dev), torch.zeros(D, dtype=bf, device=dev), \
        torch.zeros(D, dtype=bf, device=dev), torch.zeros(D, Kp, dtype=bf, device=dev)
    ln_ws = e(_hip.helper("vlr_layernorm_bwd_workspace_bytes", D), dt=torch.uint8)

    def attn_fwd():
        _hip.call("vlr_attn_fwd", qkv, qkv[:, D:], qkv[:, 2 * D:], 3 * D, o, D, lse, None, n, T, nh, hd, 0, scale)

    def attn_bwd():
        _hip.call("vlr_attn_bwd", qkv, qkv[:, D:], qkv[:, 2 * D:], 3 * D, o, do, D, lse, delta, None, dqkv, dqkv[:, D:], dqkv[:, 2 * D:], 3 * D,
                  n, T, nh, hd, 0, scale)

    def layer_fwd():
        xw.copy_(x)
        _hip.call("vlr_vit_layer_fwd", cfg, ws_, fws, xw, n, T)

    def layer_bwd():
        dx.copy_(dy)
        _hip.call("vlr_vit_layer_bwd", cfg, ws_, gs_, 0, x, bws, dx, n, T)

    def embed_bwd():
        _hip.call("vlr_vit_embed_ln_bwd", dy, pe, cls, pos, w["ln1_w"], dpe, gcls, gpos, gw, gb, 0, ln_ws, n, T, D, 1e-5)
        _hip.call("vlr_gemm_bf16", 2, dpe, patches, gpw, None, None, D, Kp, n * (T - 1), D, Kp, Kp, 0, 0, 0, 0)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(a.blocks):
            s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.reps):
                fn()
            t.record()
            torch.cuda.synchronize()
            out.append(s.elapsed_time(t) / a.reps)
        return out

    attn_fwd()
    lines = [f"vision tower backward, kernel level: {n} images x {T} tokens, D {D}, {nh} heads x {hd}, MLP {F}, {a.layers} evaluated layers; "
             f"{a.blocks} blocks x {a.reps} calls between HIP events (ms per call: block means; spread = max - min over the blocks)",
             f"device: {torch.cuda.get_device_name(0)}"]
    res = {}
    for name, fn in (("vlr_attn_fwd D=64", attn_fwd), ("vlr_attn_bwd D=64 (delta + dQ + dK,dV kernels)", attn_bwd), ("vlr_vit_layer_fwd (incl. a copy of x)", layer_fwd),
                     ("vlr_vit_layer_bwd (recompute + backward, incl. a copy of dy)", layer_bwd), ("vlr_vit_embed_ln_bwd + patch-kernel dW GEMM", embed_bwd)):
        t = timed(fn)
        res[name] = sum(t) / len(t)
        lines.append(f"{name}: " + " / ".join(f"{v:.4f}" for v in t) + f" ms, spread {max(t) - min(t):.4f} ms")
    fl = n * nh * T * T * hd
    lines.append(f"attention at D = 64: forward {4 * fl / res['vlr_attn_fwd D=64'] / 1e9:.1f} TF/s (4 B h S^2 D), backward "
                 f"{10 * fl / res['vlr_attn_bwd D=64 (delta + dQ + dK,dV kernels)'] / 1e9:.1f} TF/s (10 B h S^2 D) over the whole call")
    fwd, bwd = a.layers * res["vlr_vit_layer_fwd (incl. a copy of x)"], a.layers * res["vlr_vit_layer_bwd (recompute + backward, incl. a copy of dy)"]
    lines.append(f"per step, {a.layers} layers: ViT forward {fwd:.2f} ms, ViT backward {bwd + res['vlr_vit_embed_ln_bwd + patch-kernel dW GEMM']:.2f} ms "
                 f"(layers {bwd:.2f} + embeddings); the training pass runs one ViT forward of its own (the frozen step shares the reference's)")
    kept = (a.layers + 1) * M * D * 2
    wsb = sum(v.numel() * v.element_size() for k, v in b.items() if k != "dattn")
    lines.append(f"memory: kept layer inputs {kept / 1e6:.1f} MB, backward workspace {wsb / 1e6:.1f} MB, tower in the flat buffers "
                 f"(bf16 weights + bf16 gradients + fp32 master / m / v = 16 B per parameter): computed from shapes, not measured")
    print("\n".join(lines), flush=True)
    if not a.skip_step:
        del w, gr, fw, b, x, dy, xw, dx, qkv, do, o, dqkv, lse, delta, pe, cls, pos, dpe, patches, gcls, gpos, gw, gb, gpw, ln_ws
        lines += step_ab(a)
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
