"""Evaluation drivers on the HIP engine - the roles of the reference's src/vlrlhf/eval/utils.py (VLCollator :12-19,
load_model_and_processor :25-48, run_vqa :51-82, run_vqa_ppl :85-120).

Nothing here launches a kernel of its own: run_vqa is `model.generate` (one prefill + engine.decode_step per token on the engines with a
KV cache - Qwen-VL and InternLM-XComposer2 checkpoints are switched onto it by load_model_and_processor) and run_vqa_ppl is `model(**inputs)` + the fused lm-head log-probs of
VLDPOTrainer.get_batch_logps on the label rows, so the [B,S,V] logits are never written out.

Several GPUs are several invocations, not a collective: every entry point takes --num_shards N --shard_id i, evaluates a contiguous
range of its rows and writes `<output_path>.shard<i>`; `python -m vlrlhf.eval.merge_shards <output_path> N` joins them in order and runs
the benchmark's scoring.  Not reproduced from the reference: the MySQL reporter, accelerate, the sglang / lmdeploy variants, wandb."""
import gc
import json
import math
import os
from abc import ABC, abstractmethod
from importlib import import_module
from types import SimpleNamespace

import torch


class VLCollator(ABC):
    """a list of dataset rows -> (inputs of the model, one dict per row that the result keeps)"""

    def __init__(self, processor) -> None:
        super().__init__()
        self.processor = processor

    @abstractmethod
    def __call__(self, batch):
        raise NotImplementedError


# ---- loading -------------------------------------------------------------------------------------------------------------------
_loaded = {}            # at most ONE entry: a second checkpoint evicts the first before it is read (a 7B model does not fit twice)


def read_generation_config(model_dir):
    """generation_config.json of a checkpoint directory as a plain attribute bag (empty without the file): what the wrappers'
    prepare_default_generation_kwargs fill in and `generate` reads with getattr - transformers' GenerationConfig class is not needed"""
    cfg = SimpleNamespace()
    path = os.path.join(str(model_dir), "generation_config.json")
    if os.path.isfile(path):
        with open(path) as f:
            for k, v in json.load(f).items():
                if not k.startswith("_") and k != "transformers_version":
                    setattr(cfg, k, v)
    return cfg


def adapter_base(model_path):
    """the base checkpoint an adapter directory (LlavaForRL.save_adapter: adapter_config.json + adapter_model.safetensors) names,
    with the parsed adapter_config; (None, None) for a whole checkpoint"""
    path = os.path.join(str(model_path), "adapter_config.json")
    if not os.path.isfile(path):
        return None, None
    with open(path) as f:
        cfg = json.load(f)
    base = cfg.get("base_model_name_or_path")
    if not base:
        raise ValueError(f"{path} names no base_model_name_or_path: the adapters cannot be loaded without their base checkpoint")
    return base, cfg


def load_model_and_processor(model_path, processor_path=None, **kwargs):
    """-> (model, processor, generation_kwargs), cached for the last (model_path, processor_path).  An adapter directory loads its base
    checkpoint, applies LoRA with the saved r / alpha / targets and reads the adapter tensors; they stay un-merged (generate folds them
    into a copy of the weights per call, the perplexity forward applies them as a training forward does), which also covers a packed
    GPTQ base.  The processor then comes from the base directory unless `processor_path` says otherwise."""
    from ..utils.auto_load import MyAutoModel, MyAutoProcessor
    key = (str(model_path), str(processor_path))
    if key in _loaded:
        return _loaded[key]
    _loaded.clear()
    gc.collect()
    base, adapter_cfg = adapter_base(model_path)
    if base is not None:
        model = MyAutoModel.from_pretrained(base, **kwargs)
        model.apply_lora(adapter_cfg)
        model.load_adapter(model_path)
    else:
        model = MyAutoModel.from_pretrained(model_path, **kwargs)
    model.eval()
    if hasattr(model, "enable_kv_cache"):      # Qwen-VL, InternLM-XComposer2: answers decode from the KV cache (opt-in per model; a fresh model re-forwards)
        model.enable_kv_cache()
    config_dir = base if base is not None else model_path
    processor = MyAutoProcessor.from_pretrained(processor_path if processor_path is not None else config_dir)
    processor.infer()
    generation_kwargs = model.prepare_default_generation_kwargs(read_generation_config(config_dir))
    _loaded[key] = (model, processor, generation_kwargs)
    return _loaded[key]


def get_model_cache():
    return _loaded


# ---- the two drivers -----------------------------------------------------------------------------------------------------------
def batches(dataset, batch_size):
    """rows of `dataset` in order, `batch_size` at a time; the last batch may be short"""
    for lo in range(0, len(dataset), batch_size):
        yield [dataset[i] for i in range(lo, min(lo + batch_size, len(dataset)))]


def _on_device(inputs, model):
    dev = getattr(getattr(model, "engine", None), "dev", None)
    if dev is None:
        return inputs
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inputs.items()}


def strip_prompt(outputs, input_ids):
    """the reference's rule (:70-74): the prompt goes only when the output is longer than it AND begins with it"""
    n = input_ids.shape[1]
    if outputs.shape[1] > n and torch.equal(outputs[:, :n], input_ids.to(outputs.device)):
        return outputs[:, n:]
    return outputs


def run_vqa(model_path, dataset, collator, accelerator=None, processor_path=None, batch_size=16):
    """greedy answers: one `model.generate(**inputs, use_cache=True, **generation_kwargs)` per batch -> the rows' `others` dicts in
    dataset order, each with "response".  `accelerator` is accepted for the reference's positional order and ignored.
    `use_cache=True` is the reference's keyword; as in `generate` everywhere, a `use_cache` attribute of the generation config overrides
    it (tools/eval_bench.py selects the re-forward loop that way), and engines without a KV cache re-run the forward either way."""
    model, processor, generation_kwargs = load_model_and_processor(model_path, processor_path)
    tokenizer = processor.tokenizer
    collate = collator(processor)
    model.eval()
    results = []
    with torch.no_grad():
        for rows in batches(dataset, batch_size):
            inputs, others = collate(rows)
            inputs.pop("labels", None)
            outputs = model.generate(**inputs, use_cache=True, **generation_kwargs)
            texts = tokenizer.batch_decode(strip_prompt(outputs, inputs["input_ids"]), skip_special_tokens=True,
                                           clean_up_tokenization_spaces=False)
            for other, text in zip(others, texts):
                other["response"] = text.strip()
                results.append(other)
    return results[: len(dataset)]


def run_vqa_ppl(model_path, dataset, collator, accelerator=None, processor_path=None, batch_size=16):
    """per-row mean negative log-likelihood of the label tokens (what the reference calls ppl, :101-114) -> "ppl" in the rows' `others`
    dicts, a Python float; a row without a label gives nan, the reference's 0 / 0"""
    from ..base.trainer import VLDPOTrainer
    model, processor, _ = load_model_and_processor(model_path, processor_path)
    collate = collator(processor)
    model.eval()
    results = []
    with torch.no_grad():
        for rows in batches(dataset, batch_size):
            inputs, others = collate(rows)
            inputs = _on_device(inputs, model)
            outputs = model(**inputs)
            labels = getattr(outputs, "labels", None)          # LLaVA / LLaVA-Next: the labels of the merged (image-expanded) rows
            if labels is None:
                labels = inputs["labels"]
            nll = -VLDPOTrainer.get_batch_logps(outputs.logits, labels, average_log_prob=True)
            count = (labels[:, 1:] != -100).sum(-1).to(nll.device)
            nll = torch.where(count > 0, nll.float(), torch.full_like(nll.float(), math.nan))
            for other, v in zip(others, nll.cpu().tolist()):
                other["ppl"] = float(v)
                results.append(other)
    return results[: len(dataset)]


# ---- shards --------------------------------------------------------------------------------------------------------------------
def add_shard_args(parser):
    parser.add_argument("--num_shards", type=int, default=1, help="split the rows into this many contiguous ranges (one invocation each)")
    parser.add_argument("--shard_id", type=int, default=0)
    return parser


def shard_range(n, num_shards=1, shard_id=0):
    """rows [lo, hi) of shard `shard_id`: contiguous, in order, sizes differing by at most one (the first n % num_shards get one more)"""
    if num_shards < 1 or not 0 <= shard_id < num_shards:
        raise ValueError(f"shard_id {shard_id} is not in [0, num_shards = {num_shards})")
    q, r = divmod(n, num_shards)
    lo = shard_id * q + min(shard_id, r)
    return range(lo, lo + q + (1 if shard_id < r else 0))


class Shard:
    """the rows of one shard of a dataset (anything with __len__ and __getitem__)"""

    def __init__(self, dataset, num_shards=1, shard_id=0):
        self.dataset, self.rows = dataset, shard_range(len(dataset), num_shards, shard_id)

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, i):
        return self.dataset[self.rows[i]]


def shard_path(output_path, shard_id):
    return f"{output_path}.shard{shard_id}"


def finish(benchmark, rows, args):
    """the end of every entry point: a single invocation scores and writes `args.output_path` (the benchmark module's `finalize`); one of
    several writes its rows to `<output_path>.shard<i>` for vlrlhf.eval.merge_shards"""
    if args.num_shards == 1:
        return import_module(f"vlrlhf.eval.{benchmark}").finalize(rows, args.output_path)
    path = shard_path(args.output_path, args.shard_id)
    with open(path, "w") as f:
        json.dump(dict(benchmark=benchmark, num_shards=args.num_shards, shard_id=args.shard_id, rows=rows), f)
    print(f"[{benchmark}] shard {args.shard_id} of {args.num_shards}: {len(rows)} rows -> {path}")
    return None


def read_shards(output_path, num_shards):
    """-> (benchmark, rows of shards 0 .. num_shards-1 concatenated in order)"""
    benchmark, rows = None, []
    for i in range(num_shards):
        with open(shard_path(output_path, i)) as f:
            d = json.load(f)
        if d["num_shards"] != num_shards or d["shard_id"] != i or (benchmark is not None and d["benchmark"] != benchmark):
            raise ValueError(f"{shard_path(output_path, i)} is shard {d['shard_id']} of {d['num_shards']} of {d['benchmark']}: "
                             f"expected shard {i} of {num_shards}" + (f" of {benchmark}" if benchmark else ""))
        benchmark = d["benchmark"]
        rows.extend(d["rows"])
    return benchmark, rows
