#!/usr/bin/env python3
"""Questions per second of vlrlhf.eval.utils.run_vqa on one MI355X, KV-cache decoding against the re-forward loop.

    python tools/eval_bench.py [--questions 64] [--batch-size 16] [--new 8] [--blocks 2] [--layers 0] [--out profiles/eval_throughput.txt]

Set-up: a POPE-shaped synthetic set - 64 prompts of 52 to 68 text tokens (unequal on purpose: every batch is left-padded) with one 336^2
image each - answered greedily by the in-memory 7B LLaVA-1.5 of bench.py's recipe (utils/synthetic init_hashed_model), batches of 16,
answers capped at 8 new tokens, no stop before the cap.  One pass is one run_vqa call over the whole set: collate, generate, strip the
prompt, decode the tokens.  Tokenising text and decoding image files are NOT in it (the rows carry ids and pixel tensors).
The two routes alternate in one process, cached first, `--blocks` passes each after one warm-up pass each; a pass is timed by the wall clock
around run_vqa with a device synchronisation on both sides.  The yardstick of the cached route is the re-forward loop of the same run."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vl-rlhf_amd"))
sys.path.insert(0, ROOT)


def synthetic_questions(n, cfg, seed=1234):
    """rows of a POPE-like set: BOS, one <image> at index 4, 52 - 68 ids in all; a 336^2 CLIP-normalised random image"""
    from vlrlhf.utils.synthetic import synthetic_pixels
    g = torch.Generator().manual_seed(seed)
    px = synthetic_pixels(n, cfg["image_size"], seed)
    rows = []
    for i in range(n):
        T = 52 + int(torch.randint(0, 17, (1,), generator=g))
        ids = torch.randint(3, 32000, (T,), generator=g)
        ids[0], ids[4] = 1, cfg["image_token"]
        rows.append(dict(ids=ids, pixels=px[i], label="yes" if i % 2 else "no"))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=64)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--new", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--layers", type=int, default=0, help="fewer decoder layers (a dry run; the result is then marked)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench.py measures on the MI355X: no GPU here")
    import vlrlhf.eval.utils as U
    from vlrlhf.models.Llava import LlavaForRL
    from vlrlhf.utils.synthetic import LLAVA_1_5_7B, init_hashed_model
    cfg = dict(LLAVA_1_5_7B)
    if a.layers:
        cfg["layers"] = a.layers
    model = LlavaForRL(cfg)
    init_hashed_model(model, seed=0, std=0.02, policy_delta=1e-3)
    model.eval()
    rows = synthetic_questions(a.questions, cfg)

    class Collator(U.VLCollator):
        def __call__(self, batch):
            n = max(len(b["ids"]) for b in batch)
            ids = torch.zeros(len(batch), n, dtype=torch.long)
            mask = torch.zeros_like(ids)
            for r, b in enumerate(batch):
                ids[r, n - len(b["ids"]):] = b["ids"]
                mask[r, n - len(b["ids"]):] = 1
            return dict(input_ids=ids, attention_mask=mask, pixel_values=torch.stack([b["pixels"] for b in batch])), \
                [dict(label=b["label"]) for b in batch]

    tokenizer = SimpleNamespace(batch_decode=lambda ids, **k: [" ".join(map(str, row)) for row in ids.tolist()])
    gen = SimpleNamespace(max_new_tokens=a.new, do_sample=False, eos_token_id=10 ** 6, pad_token_id=0, use_cache=True)
    U.load_model_and_processor = lambda *x, **k: (model, SimpleNamespace(tokenizer=tokenizer), dict(generation_config=gen))

    def one_pass(use_cache):
        gen.use_cache = use_cache
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = U.run_vqa("synthetic", rows, Collator, None, None, a.batch_size)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert len(out) == len(rows) and all(len(o["response"].split()) == a.new for o in out)
        return dt, [o["response"] for o in out]

    answers = {}
    for route in (True, False):                     # warm-up: code objects, workspaces, the vision cache's shapes
        answers[route] = one_pass(route)[1]
    times = {True: [], False: []}
    for _ in range(a.blocks):
        for route in (True, False):
            times[route].append(one_pass(route)[0])
    same = sum(x == y for x, y in zip(answers[True], answers[False]))
    first = sum(x.split()[0] == y.split()[0] for x, y in zip(answers[True], answers[False]))
    qps = {r: [a.questions / t for t in ts] for r, ts in times.items()}
    res = dict(questions=a.questions, batch_size=a.batch_size, new_tokens=a.new, layers=model.engine.L, full_depth=not a.layers,
               kv_cache_s=[round(t, 3) for t in times[True]], reforward_s=[round(t, 3) for t in times[False]],
               kv_cache_qps=[round(q, 2) for q in qps[True]], reforward_qps=[round(q, 2) for q in qps[False]],
               speedup=round(min(times[False]) / min(times[True]), 2), identical_answers=same, identical_first_tokens=first)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("run_vqa throughput on one MI355X (tools/eval_bench.py; synthetic 7B LLaVA-1.5, greedy answers)\n\n")
            patches = (cfg["image_size"] // cfg["patch_size"]) ** 2      # the <image> id is REPLACED by the patch rows: T - 1 + patches merged rows
            lens = [len(r["ids"]) for r in rows]
            f.write(f"{a.questions} POPE-shaped questions: {min(lens)} - {max(lens)} text tokens + one {cfg['image_size']}^2 image "
                    f"({min(lens) - 1 + patches} - {max(lens) - 1 + patches} merged rows), left-padded batches of "
                    f"{a.batch_size}, {a.new} new tokens each, {model.engine.L} decoder layers{'' if not a.layers else ' (NOT the 7B depth)'}.\n")
            f.write("One pass = one run_vqa call over the set (collate, generate, strip, decode); wall clock, device synchronised on both sides;\n")
            f.write(f"the routes alternate in one process after one warm-up pass each, {a.blocks} passes each.\n\n")
            f.write("route                         seconds per pass        questions per second\n")
            for name, r in (("use_cache=True  (KV cache)  ", True), ("use_cache=False (re-forward)", False)):
                f.write(f"{name}  {'  '.join(f'{t:7.3f}' for t in times[r]):22s}  {'  '.join(f'{q:7.2f}' for q in qps[r])}\n")
            f.write(f"\nspeed-up of the cached route (best pass of each): {res['speedup']} x\n")
            f.write(f"answers identical between the routes: {same} of {a.questions}; first tokens identical: {first} of {a.questions} "
                    "(the first token comes from the same prefill; later ones differ by the decode kernels' rounding on random weights)\n")
    return res


if __name__ == "__main__":
    main()
