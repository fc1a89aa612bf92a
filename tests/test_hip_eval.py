"""vlrlhf.eval on the MI355X: perplexities of right-padded option rows against the committed fp32 golden logits (all four families), the
option they select, run_vqa over left-padded prompts of unequal length on the KV-cache route (LLaVA) and the re-forward route (Qwen-VL),
stop sequences on both routes, an adapter directory, and the POPE / SEED-Bench entry points in a child process.
Needs a real MI355X:  pytest -m gpu

The perplexity fixture of the LLaVA family is llava_hipsmall, the fixture test_forward_matches_golden and TOL_CE speak of: the engine
refuses llava_tiny (decoder head_dim 12; the gfx950 attention kernels take 128)."""
import functools
import itertools
import json
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests.golden_util import load_case, t, write_tiny_checkpoint  # noqa: E402
from tests.qwen_standin import StandInTokenizer  # noqa: E402
from tests.test_hip_sft import TOL_CE, _family, sft_inputs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ["llava", "llavanext", "qwenvl", "internlm"]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return torch.device("cuda")


class patched_loader:
    """utils.load_model_and_processor answering with an in-memory model (the fixtures are tensors, not checkpoint directories)"""

    def __init__(self, model, processor, generation_kwargs=None):
        self.answer = (model, processor, generation_kwargs or {})

    def __enter__(self):
        import vlrlhf.eval.utils as U
        self.U, self.saved = U, U.load_model_and_processor
        U.load_model_and_processor = lambda *a, **k: self.answer
        return U

    def __exit__(self, *exc):
        self.U.load_model_and_processor = self.saved


# ------------------------------------------------------------------------------------------------------------ 1, 2  perplexity
def golden_nll(logits, labels):
    """per-row mean cross-entropy of the golden fp32 logits over the (merged) labels, in fp64: what the reference's run_vqa_ppl computes"""
    out = []
    for row_logits, row_labels in zip(logits[:, :-1], labels[:, 1:]):
        sel = row_labels != -100
        out.append(float(F.cross_entropy(row_logits[sel].double(), row_labels[sel])))
    return out


def keep_first_label(labels, row):
    first = int((labels[row] != -100).nonzero()[0])
    labels[row, first + 1:] = -100


@functools.lru_cache(maxsize=None)
def scored(family):
    """one run_vqa_ppl over the family's fixture - its four right-padded rows in one batch, as the golden logits were made - and the
    golden values -> (hip ppl per row, golden ppl per row, label tokens per row).  LLaVA: row 0 keeps ONE label token."""
    from vlrlhf.eval.utils import VLCollator
    dev = torch.device("cuda")
    if family == "llava":
        from tests.test_hip_e2e import build
        z, cfg, W, W_ref, batch, _ = load_case("llava_hipsmall")
        model, _ = build(cfg, W, W_ref)
        inp = sft_inputs(cfg, batch, dev)
        merged = t(z, "merged_labels").clone()
        inp["labels"] = inp["labels"].clone()
        keep_first_label(inp["labels"], 0)
        keep_first_label(merged, 0)
    else:
        z, model, tr, batch, merged, _ = _family(family)
        cb = tr.concatenated_inputs(batch, device=dev)
        inp = dict(input_ids=cb["concatenated_input_ids"], attention_mask=cb["concatenated_attention_mask"], labels=cb["concatenated_labels"],
                   **cb["concatenated_img_input_dict"])
        merged = merged if merged is not None else cb["concatenated_labels"].cpu()
    n = inp["input_ids"].shape[0]
    assert bool((inp["attention_mask"][:, -1] == 0).any()) and bool((inp["attention_mask"][:, 0] == 1).all()), "right-padded rows"

    class Rows(VLCollator):
        def __call__(self, rows):
            idx = torch.tensor([r["row"] for r in rows], device=dev)
            inputs = {k: (v[idx] if isinstance(v, torch.Tensor) and v.shape[0] == n else v) for k, v in inp.items()}
            return inputs, [dict(row=r["row"]) for r in rows]

    with patched_loader(model, None) as U:
        out = U.run_vqa_ppl("fixture", [dict(row=i) for i in range(n)], Rows, None, None, 16)
    assert [o["row"] for o in out] == list(range(n)) and all(isinstance(o["ppl"], float) for o in out)
    counts = (merged[:, 1:] != -100).sum(1).tolist()
    return [o["ppl"] for o in out], golden_nll(t(z, "logits"), merged), counts


@pytest.mark.parametrize("family", FAMILIES)
def test_run_vqa_ppl_matches_golden_cross_entropy(gpu, family):
    hip, gold, counts = scored(family)
    for i, (h, g, c) in enumerate(zip(hip, gold, counts)):
        print(f"[eval ppl] {family} row {i}: {c} label tokens  hip={h:.6f}  golden fp32={g:.6f}  |diff|={abs(h - g):.2e}  (bound {TOL_CE})")
    if family == "llava":
        assert counts[0] == 1 and min(counts[1:]) >= 2, "one label token: the smallest count an average can go wrong at"
    assert all(math.isfinite(h) for h in hip)
    for h, g in zip(hip, gold):
        assert abs(h - g) < TOL_CE, (family, hip, gold)


def questions(n):
    """the fixture's rows as multiple-choice questions: every pair of rows, every three, and all of them (option = row)"""
    return [rows for k in range(2, n + 1) for rows in itertools.combinations(range(n), k)]


@pytest.mark.parametrize("family", FAMILIES)
def test_selected_option_matches_golden_where_the_margin_allows(gpu, family):
    """a question whose two best golden values are more than 10 x TOL_CE apart cannot flip under an error below TOL_CE per row"""
    from vlrlhf.eval.seedbench.eval import pick_answers
    hip, gold, _ = scored(family)
    qualified = 0
    for q in questions(len(gold)):
        best = sorted(gold[r] for r in q)
        if best[1] - best[0] <= 10 * TOL_CE:
            continue
        qualified += 1
        as_rows = lambda vals: [dict(question_id="q", choice=r, ppl=vals[r]) for r in q]      # noqa: E731
        assert pick_answers(as_rows(hip))["q"]["choice"] == pick_answers(as_rows(gold))["q"]["choice"], (family, q, hip, gold)
    print(f"[eval argmin] {family}: {qualified} of {len(questions(len(gold)))} questions have a golden margin above {10 * TOL_CE}")
    assert qualified >= 1, f"{family}: no question of the fixture has a golden margin above {10 * TOL_CE}"


# ------------------------------------------------------------------------------------------------------------ 3, 4  generation
QUESTIONS = [dict(image="im0.png", prompt="Is there a cat in the photo?", label="no"),
             dict(image="im1.png", prompt="Is there a small brown dog running across the green field in the image?", label="yes")]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    """a tiny LLaVA checkpoint (with its processor files) and two pictures"""
    from PIL import Image
    d = tmp_path_factory.mktemp("eval")
    write_tiny_checkpoint(str(d / "ckpt"))
    for name, colour in (("im0.png", (200, 40, 40)), ("im1.png", (40, 40, 200))):
        Image.new("RGB", (40, 32), colour).save(d / name)
    return d


class SmallQwenTokenizer(StandInTokenizer):
    """StandInTokenizer in the id space of the qwenvl_small fixture (vocabulary 520, 16 image slots)"""
    im_start_id, im_end_id, eod_id = 511, 512, 510
    img_start_id, img_end_id, img_pad_id = 500, 501, 502
    SPECIAL = {"<|im_start|>": 511, "<|im_end|>": 512, "<|endoftext|>": 510}
    SLOTS = 16

    def __call__(self, text):
        ids = []
        for part in self._SPLIT.split(text):
            if not part:
                continue
            if part in self.SPECIAL:
                ids.append(self.SPECIAL[part])
            elif part.startswith("<img>") and part.endswith("</img>"):
                b = list(part[5:-6].encode("utf-8"))
                assert len(b) < self.SLOTS - 1
                ids += [self.img_start_id] + b + [self.img_pad_id] * (self.SLOTS - len(b)) + [self.img_end_id]
            else:
                ids += [ord(c) % 200 + 256 for c in part]
        return SimpleNamespace(input_ids=ids, attention_mask=[1] * len(ids))

    def batch_decode(self, rows, skip_special_tokens=False, clean_up_tokenization_spaces=None):
        return ["".join(chr(32 + (int(i) - 256) % 95) if 256 <= int(i) < 456 else ("" if skip_special_tokens else f"<{int(i)}>") for i in row)
                for row in rows]


def llava_route(workdir):
    from vlrlhf.eval.utils import load_model_and_processor
    model, proc, kw = load_model_and_processor(str(workdir / "ckpt"))
    assert model.engine.supports_kv_cache and model.engine.hd == 128
    kw["generation_config"].max_new_tokens = 8          # (the wrapper's default is 1024; the cached entry keeps this object)
    rows = [dict(q, image=str(workdir / q["image"])) for q in QUESTIONS]
    return model, proc, kw, rows


def qwen_route():
    from vlrlhf.models.QwenVL import QwenVLForRL, QwenVLProcessor
    z, cfg, W, W_ref, batch, _ = load_case("qwenvl_small")
    model = QwenVLForRL.from_state_dict(cfg, W)
    assert not model.engine.supports_kv_cache
    proc = QwenVLProcessor(tokenizer=SmallQwenTokenizer(), image_size=cfg["visual"]["image_size"])
    proc.infer()
    kw = model.prepare_default_generation_kwargs(SimpleNamespace(max_new_tokens=8, eos_token_id=10 ** 6))
    return model, proc, kw, [dict(q) for q in QUESTIONS]       # image names relative to the working directory: <= 14 bytes fit the slots


def collate(proc, rows):
    from vlrlhf.eval.pope.eval import Collator
    inputs, others = Collator(proc)([dict(r) for r in rows])
    inputs.pop("labels", None)
    m = inputs["attention_mask"]
    assert m.shape[0] == 2 and int(m[0].sum()) != int(m[1].sum()) and bool((m[:, 0] == 0).any()) and bool((m[:, -1] == 1).all()), \
        "two prompts of different length, left-padded"
    return inputs


@pytest.mark.parametrize("route", ["llava_kv_cache", "qwen_reforward"])
def test_run_vqa_equals_direct_greedy_generate(gpu, workdir, monkeypatch, route):
    from vlrlhf.eval.pope.eval import Collator
    monkeypatch.chdir(workdir)
    model, proc, kw, rows = llava_route(workdir) if route.startswith("llava") else qwen_route()
    steps = []
    ds = model.engine.decode_step
    monkeypatch.setattr(model.engine, "decode_step", lambda *a, **k: (steps.append(1), ds(*a, **k))[1])
    inputs = collate(proc, rows)
    direct = model.generate(**inputs, use_cache=True, **kw)
    n = inputs["input_ids"].shape[1]
    assert direct.shape[1] > n and torch.equal(direct[:, :n].cpu(), inputs["input_ids"])
    want = [s.strip() for s in proc.tokenizer.batch_decode(direct[:, n:], skip_special_tokens=True, clean_up_tokenization_spaces=False)]
    assert (len(steps) > 0) == route.startswith("llava"), "LLaVA decodes from the KV cache, Qwen-VL re-runs the forward"
    with patched_loader(model, proc, kw) as U:
        out = U.run_vqa("fixture", rows, Collator, None, None, 16)
    print(f"[eval run_vqa] {route}: {[o['response'] for o in out]}")
    assert [o["response"] for o in out] == want and [o["label"] for o in out] == ["no", "yes"]


@pytest.mark.parametrize("route", ["llava_kv_cache", "qwen_reforward"])
def test_stop_sequence_ends_one_row_and_leaves_the_other(gpu, workdir, monkeypatch, route):
    monkeypatch.chdir(workdir)
    model, proc, _, rows = llava_route(workdir) if route.startswith("llava") else qwen_route()
    inputs = collate(proc, rows)
    n, new, pad = inputs["input_ids"].shape[1], 8, 3
    free = model.generate(**inputs, max_new_tokens=new, do_sample=False, eos_token_id=10 ** 6, pad_token_id=pad)[:, n:].cpu()
    assert free.shape == (2, new)
    stop = free[0, 2:4].tolist()
    gc = SimpleNamespace(stop_words_ids=[stop], max_new_tokens=new, do_sample=False, eos_token_id=10 ** 6, pad_token_id=pad)
    got = model.generate(**inputs, generation_config=gc)[:, n:].cpu()
    # the rule, restated on the unconstrained stream: a row ends at the first position k >= 1 whose tokens k-1, k are the stop sequence
    want = free.clone()
    ends = []
    for r in range(2):
        hits = [k for k in range(1, new) if free[r, k - 1:k + 1].tolist() == stop]
        ends.append(hits[0] if hits else None)
        if hits:
            want[r, hits[0] + 1:] = pad
    print(f"[eval stop] {route}: stop {stop}; unconstrained {free.tolist()}; constrained {got.tolist()}; rows end at {ends}")
    # the scenario itself, not only the rule: with these weights and prompts (bit-reproducible kernels) row 0's tokens 2-3 occur nowhere
    # earlier in row 0 and nowhere in row 1, so row 0 ends at token 3 and row 1 never does
    assert ends == [3, None], (stop, free.tolist())
    assert got.shape[1] == new
    assert torch.equal(got[0, :4], free[0, :4]) and bool((got[0, 4:] == pad).all()), "row 0: unchanged up to and including token 3, pad after"
    assert torch.equal(got[1], free[1]), "row 1 token for token unchanged"
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------------------ 5  adapter directory
def test_adapter_directory_generates_like_the_in_memory_model(gpu, workdir):
    from vlrlhf.eval.utils import get_model_cache, load_model_and_processor
    from vlrlhf.models.Llava import LlavaForRL
    ckpt, ad = str(workdir / "ckpt"), str(workdir / "adapter")
    model = LlavaForRL.from_pretrained(ckpt)
    model.apply_lora(dict(r=8, lora_alpha=16, lora_dropout=0.0, target_modules="auto", bias="none"))
    g = torch.Generator().manual_seed(5)
    for v in model.engine.lv.values():                       # non-zero lora_B: the adapters change the tokens' logits
        v.copy_((torch.randn(v.shape, generator=g) * 0.05).to(v.dtype))
    model.eval()
    model.save_adapter(ad, base_model_name_or_path=ckpt)
    get_model_cache().clear()
    loaded, proc, kw = load_model_and_processor(ad)
    assert loaded is not model and loaded.engine.lora is not None and loaded.cached_lora_route() == "merged"
    assert torch.equal(loaded.engine.lora_flat, model.engine.lora_flat) and torch.equal(loaded.engine.policy.flat, model.engine.policy.flat)
    inputs = collate(proc, [dict(q, image=str(workdir / q["image"])) for q in QUESTIONS])
    run = lambda m, **k: m.generate(**inputs, max_new_tokens=6, do_sample=False, eos_token_id=10 ** 6, pad_token_id=0, **k).cpu()      # noqa: E731
    assert torch.equal(run(loaded), run(model))
    with model.disable_adapter():
        base = run(model, use_cache=False)
    live = run(model, use_cache=False)
    assert torch.equal(run(loaded, use_cache=False), live)
    assert not torch.equal(base, live), "the adapters change the greedy tokens: a generate that ignored them would pass everything above"
    print(f"[eval adapter] with adapters {live[:, -6:].tolist()}  base {base[:, -6:].tolist()}")
    get_model_cache().clear()


# ------------------------------------------------------------------------------------------------------------ 6  entry points
def child(module, *args):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "vl-rlhf_amd"), ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-m", module, *map(str, args)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def test_pope_entry_point_in_a_child_process(workdir, tmp_path):
    os.makedirs(tmp_path / "questions")
    for name, labels in (("coco_pope_random.json", ("yes", "no", "yes")), ("coco_pope_adversarial.json", ("no", "yes", "no"))):
        with open(tmp_path / "questions" / name, "w") as f:
            for i, label in enumerate(labels):
                f.write(json.dumps(dict(question_id=i, image=f"im{i % 2}.png", text=QUESTIONS[i % 2]["prompt"], label=label)) + "\n")
    out = tmp_path / "pope.json"
    child("vlrlhf.eval.pope.eval", "--image_root", workdir, "--file_root", tmp_path / "questions", "--model_path", workdir / "ckpt",
          "--output_path", out, "--batch_size", 4)
    d = json.load(open(out))
    assert len(d["results"]) == 6 and all({"response", "label", "category"} <= set(r) and isinstance(r["response"], str) for r in d["results"])
    assert sorted({r["category"] for r in d["results"]}) == ["coco_pope_adversarial.json", "coco_pope_random.json"] == sorted(d["metrics"])
    for m in d["metrics"].values():
        assert set(m) == {"acc", "precision", "recall", "f1", "yes_rate"} and all(0.0 <= v <= 100.0 for v in m.values())


def test_seedbench_entry_point_in_a_child_process(workdir, tmp_path):
    import shutil
    os.makedirs(tmp_path / "SEED-Bench-image")
    for name in ("im0.png", "im1.png"):
        shutil.copy(workdir / name, tmp_path / "SEED-Bench-image" / name)
    qs = [dict(question_id="11", question_type_id=1, data_id="im0.png", question="What colour is the car?", choice_a="red", choice_b="green",
               choice_c="brown", choice_d="white", answer="A"),
          dict(question_id="12", question_type_id=10, data_id="clip.mp4", question="What happens?", choice_a="a", choice_b="b", choice_c="c",
               choice_d="d", answer="A"),
          dict(question_id="13", question_type_id=5, data_id="im1.png", question="How many apples are on the table?", choice_a="one apple",
               choice_b="There are three apples", choice_c="two", choice_d="no apples at all", answer="B")]
    with open(tmp_path / "SEED-Bench.json", "w") as f:
        json.dump(dict(question_type={"Scene Understanding": 1, "Instance Counting": 5, "Action Recognition": 10}, questions=qs), f)
    out = tmp_path / "seed.json"
    child("vlrlhf.eval.seedbench.eval", "--data_root", tmp_path, "--model_path", workdir / "ckpt", "--output_path", out, "--batch_size", 3)
    d = json.load(open(out))
    assert sorted(d) == ["11", "13"], "two image questions (eight rows), the video question filtered out"
    assert all(a["choice"] in "ABCD" and math.isfinite(a["ppl"]) and 0.0 < a["ppl"] < 20.0 for a in d.values())
    from vlrlhf.eval.seedbench.calculate import calculate
    acc = calculate(str(out), str(tmp_path / "SEED-Bench.json"), "image")
    assert set(acc) == {"SceneUnderstanding", "InstanceCounting", "Total"}
