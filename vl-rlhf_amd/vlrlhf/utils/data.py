"""Dataset builders -> rows {prompt, chosen, rejected, img_path} (mirror of /root/reference/src/vlrlhf/utils/data.py:
DATASET_MAP :142-147).  The reference downloads vlfeedback_paired / rlhfv from the HuggingFace hub; there is no network here, so
those two read a local export of the same rows (`--data_path`) and run the reference's pair mining on it; `plain_dpo` and
`vlquery_json` read the same JSON formats as the reference and `synthetic` generates VLFeedback-shaped rows for benchmarks."""
import json
import os

import torch


def make_plain_dpo_dataset(script_args):
    with open(script_args.data_path) as f:
        data = json.load(f)
    rows = []
    for d in data:
        img = d["image"] if "image" in d else d["img_path"]
        if getattr(script_args, "image_root", None):
            img = os.path.join(script_args.image_root, img)
        rows.append(dict(prompt=d["prompt"], chosen=d["chosen"], rejected=d["rejected"], img_path=img))
    return rows


def make_synthetic_dataset(script_args):
    n = int(getattr(script_args, "synthetic_rows", 64))
    size = int(getattr(script_args, "synthetic_image_size", 336))
    g = torch.Generator().manual_seed(1234)
    words = ["alpha", "beta", "gamma", "delta", "red", "blue", "cat", "dog", "tree", "car", "sky", "left", "right"]

    def sent(k):
        return " ".join(words[int(i)] for i in torch.randint(0, len(words), (k,), generator=g))
    rows = []
    for _ in range(n):
        rows.append(dict(prompt="What is shown? " + sent(6), chosen=sent(int(torch.randint(4, 24, (1,), generator=g))),
                         rejected=sent(int(torch.randint(4, 24, (1,), generator=g))),
                         img_path=torch.randn(3, size, size, generator=g)))
    return rows


def make_synthetic_conversations_dataset(script_args):
    """`--dataset_name synthetic_conversations`: vlquery_json-shaped SFT rows {conversations, image, img_path} for tests and benchmarks.
    Every row has two or three user / assistant turns; every assistant turn but the last ends with the literal "</s>", as chat exports
    that keep the end-of-turn token do - those are the eos tokens INSIDE a conversation that VLSFTTrainer.tokenize_row masks out of
    attention and labels (the holes in the key mask)."""
    n = int(getattr(script_args, "synthetic_rows", 64))
    size = int(getattr(script_args, "synthetic_image_size", 336))
    g = torch.Generator().manual_seed(4321)
    words = ["alpha", "beta", "gamma", "delta", "red", "blue", "cat", "dog", "tree", "car", "sky", "left", "right"]

    def sent(k):
        return " ".join(words[int(i)] for i in torch.randint(0, len(words), (k,), generator=g))
    rows = []
    for r in range(n):
        turns = 2 + r % 2
        conv = []
        for t in range(turns):
            conv.append({"from": "user", "value": ("What is shown? " if t == 0 else "And then? ") + sent(4)})
            conv.append({"from": "assistant", "value": sent(int(torch.randint(3, 12, (1,), generator=g))) + ("</s>" if t + 1 < turns else "")})
        rows.append(dict(conversations=conv, image=f"synthetic_{r}", img_path=torch.randn(3, size, size, generator=g)))
    return rows


def _load_rows(path):
    """a local export of a hub dataset: .json (list), .jsonl, or a directory of such files"""
    files = [os.path.join(path, f) for f in sorted(os.listdir(path))] if os.path.isdir(path) else [path]
    rows = []
    for fn in files:
        if fn.endswith(".jsonl"):
            with open(fn) as f:
                rows += [json.loads(l) for l in f if l.strip()]
        elif fn.endswith(".json"):
            with open(fn) as f:
                d = json.load(f)
            rows += d if isinstance(d, list) else [d]
    return rows


def vlfeedback_pairs(samples, score_margin=-1):
    """reference utils/data.py:16-71 (`make_batch_pairs`): every pair of completions of a sample is ordered by the MEAN of the
    annotators' per-aspect `Rating`s (pairs with an unparsable rating or a tie are skipped); score_margin == -1 keeps only the
    pairs with the LARGEST gap of the sample, otherwise every pair whose gap >= score_margin.  -> rows {prompt, chosen, rejected, img_path}"""
    from itertools import combinations
    out = []
    for s in samples:
        comps = s["completions"]
        by_gap = {}
        for i, j in combinations(range(len(comps["annotations"])), 2):
            a1, a2 = comps["annotations"][i], comps["annotations"][j]
            try:
                s1 = sum(float(a1[k]["Rating"]) for k in a1) / len(a1)
                s2 = sum(float(a2[k]["Rating"]) for k in a2) / len(a2)
            except ValueError:
                continue
            if s1 == s2:
                continue
            c, r = (i, j) if s1 > s2 else (j, i)
            by_gap.setdefault(abs(s1 - s2), []).append(dict(prompt=s["prompt"], chosen=comps["response"][c], rejected=comps["response"][r],
                                                               img_path=s["img_path"]))
        if not by_gap:
            continue
        if score_margin == -1:
            out += by_gap[max(by_gap)]
        else:
            for gap, rows in by_gap.items():       # insertion order = the order the reference's defaultdict saw the gaps
                if gap >= score_margin:
                    out += rows
    return out


def make_vlfeedback_paired_dataset(script_args):
    """reference :11-82.  The hub dataset MMInstruction/VLFeedback cannot be downloaded here: `--data_path` names a local export
    of its rows ({prompt, img_path, completions: {annotations: [...], response: [...]}}; .json / .jsonl / directory)."""
    path = getattr(script_args, "data_path", None)
    if not path:
        raise RuntimeError("dataset 'vlfeedback_paired' is downloaded from the HuggingFace hub by the reference; there is no network "
                           "here - pass --data_path <local export of MMInstruction/VLFeedback rows>")
    rows = _load_rows(path)
    root = getattr(script_args, "image_root", None)
    if root:
        for r in rows:
            r["img_path"] = os.path.join(root, r["img_path"])
    return vlfeedback_pairs(rows, getattr(script_args, "score_margin", -1))


def make_rlhfv_paired_dataset(script_args):
    """reference :100-117: rows {image_path, text: json{question, chosen, rejected}} of a local export of HaoyeZhang/RLHF-V-Dataset"""
    path = getattr(script_args, "data_path", None)
    if not path:
        raise RuntimeError("dataset 'rlhfv' is downloaded from the HuggingFace hub by the reference; pass --data_path <local export>")
    out = []
    for r in _load_rows(path):
        t = json.loads(r["text"]) if isinstance(r["text"], str) else r["text"]
        out.append(dict(img_path=os.path.join(script_args.image_root or "", r["image_path"]), prompt=t["question"], chosen=t["chosen"],
                        rejected=t["rejected"]))
    return out


def build_dataset_from_vlquery_json(script_args):
    """reference :85-97: a JSON list whose rows carry `image`; img_path = image_root / image, everything else passes through"""
    with open(script_args.data_path) as f:
        raw = json.load(f)
    return [dict(d, img_path=os.path.join(script_args.image_root or "", d["image"])) for d in raw]


def unpair(rows):
    """paired rows {prompt, chosen, rejected, img_path} -> KTO's unpaired rows {prompt, completion, label, img_path}: every pair gives
    (prompt, chosen, True) then (prompt, rejected, False), both with the pair's prompt and img_path"""
    out = []
    for r in rows:
        out.append(dict(prompt=r["prompt"], completion=r["chosen"], label=True, img_path=r["img_path"]))
        out.append(dict(prompt=r["prompt"], completion=r["rejected"], label=False, img_path=r["img_path"]))
    return out


def make_kto_json_dataset(script_args):
    """`--dataset_name kto_json`: a JSON list of {prompt, completion, label, image | img_path} - one prompt, one completion and one
    thumbs-up (true) or thumbs-down (false) per row; img_path = image_root / image"""
    with open(script_args.data_path) as f:
        data = json.load(f)
    rows = []
    for d in data:
        img = d["image"] if "image" in d else d["img_path"]
        if getattr(script_args, "image_root", None):
            img = os.path.join(script_args.image_root, img)
        label = d["label"]
        if isinstance(label, str):
            label = label.strip().lower() in ("1", "true", "yes")
        rows.append(dict(prompt=d["prompt"], completion=d["completion"], label=bool(label), img_path=img))
    return rows


def make_vlfeedback_unpaired_dataset(script_args):
    return unpair(make_vlfeedback_paired_dataset(script_args))


def make_rlhfv_unpaired_dataset(script_args):
    return unpair(make_rlhfv_paired_dataset(script_args))


def make_synthetic_unpaired_dataset(script_args):
    """`--dataset_name synthetic_unpaired`: the synthetic pairs split in two (tests, benchmarks)"""
    return unpair(make_synthetic_dataset(script_args))[: int(getattr(script_args, "synthetic_rows", 64))]


DATASET_MAP = {
    "kto_json": make_kto_json_dataset,
    "vlfeedback_unpaired": make_vlfeedback_unpaired_dataset,
    "rlhfv_unpaired": make_rlhfv_unpaired_dataset,
    "synthetic_unpaired": make_synthetic_unpaired_dataset,
    "vlfeedback_paired": make_vlfeedback_paired_dataset,
    "rlhfv": make_rlhfv_paired_dataset,
    "vlquery_json": build_dataset_from_vlquery_json,
    "plain_dpo": make_plain_dpo_dataset,
    "synthetic": make_synthetic_dataset,
    "synthetic_conversations": make_synthetic_conversations_dataset,
}
