"""DPO, SFT and reward-model collators (mirror of the reference src/vlrlhf/base/collator.py:8-111)."""
from dataclasses import dataclass
from typing import Any, Dict, List, Optional

import torch


@dataclass
class VLDPODataCollatorWithPadding:
    r"""Pads the tokenized rows of a DPO batch: chosen_/rejected_ on the right, prompt_ on the left;
    ids -> pad_token_id, labels -> label_pad_token_id, masks -> 0; `*_logps` become a float tensor (cached reference
    log-probs); every other key is passed through as a list."""

    pad_token_id: int = 0
    label_pad_token_id: int = -100
    is_encoder_decoder: Optional[bool] = False
    processor: Optional[Any] = None

    def __call__(self, features: List[Dict[str, Any]]) -> Dict[str, Any]:
        if self.is_encoder_decoder:
            raise NotImplementedError("encoder-decoder models are not on the MI355X DPO path")
        out: Dict[str, Any] = {}
        for k in features[0].keys():
            if k.endswith("_input_ids") or k.endswith("_attention_mask") or k.endswith("_labels"):
                if k.endswith("_input_ids"):
                    pad = self.pad_token_id
                elif k.endswith("_labels"):
                    pad = self.label_pad_token_id
                elif k.endswith("_attention_mask"):
                    pad = 0
                else:
                    raise ValueError(f"Unexpected key in batch '{k}'")
                n = max(len(f[k]) for f in features)
                t = torch.full((len(features), n), pad, dtype=torch.long)
                left = "prompt" in k
                for i, f in enumerate(features):
                    v = torch.as_tensor(f[k], dtype=torch.long)
                    if left:
                        t[i, n - v.numel():] = v
                    else:
                        t[i, : v.numel()] = v
                out[k] = t
            elif k.endswith("_logps"):
                out[k] = torch.tensor([f[k] for f in features])
            else:
                out[k] = [f[k] for f in features]
        return out


@dataclass
class VLSFTDataCollatorWithPadding:
    r"""reference :70-94: right-pads input_ids -> pad_token_id, labels -> label_pad_token_id, attention_mask -> 0 (the padding of
    torch pad_sequence(batch_first=True)); `img_path` is passed through as a list; any other key raises."""

    pad_token_id: int
    label_pad_token_id: int
    processor: Optional[Any] = None

    def __call__(self, features: List[Dict[str, Any]]) -> Dict[str, Any]:
        out: Dict[str, Any] = {}
        for k in features[0].keys():
            if k == "img_path":
                out[k] = [f[k] for f in features]
                continue
            if k == "input_ids":
                pad = self.pad_token_id
            elif k == "labels":
                pad = self.label_pad_token_id
            elif k == "attention_mask":
                pad = 0
            else:
                raise ValueError(f"Unexpected key in batch '{k}'")
            n = max(len(f[k]) for f in features)
            t = torch.full((len(features), n), pad, dtype=torch.long)
            for i, f in enumerate(features):
                v = torch.as_tensor(f[k], dtype=torch.long)
                t[i, : v.numel()] = v
            out[k] = t
        return out


@dataclass
class VLRMDataCollatorWithPadding:
    r"""reference :96-111: right-pads input_ids_* -> pad_token_id and attention_mask_* -> 0 (torch pad_sequence(batch_first=True)), each
    key to its own width; any other key raises.  Deliberate difference: `img_path` is passed through as a list - the reference's
    tokenize_row drops it, so as shipped only a model that reads the path out of the text ever sees its image."""

    pad_token_id: int
    processor: Optional[Any] = None

    def __call__(self, features: List[Dict[str, Any]]) -> Dict[str, Any]:
        out: Dict[str, Any] = {}
        for k in features[0].keys():
            if k == "img_path":
                out[k] = [f[k] for f in features]
                continue
            if k.startswith("input_ids"):
                pad = self.pad_token_id
            elif k.startswith("attention_mask"):
                pad = 0
            else:
                raise ValueError(f"Unexpected key in batch '{k}'")
            n = max(len(f[k]) for f in features)
            t = torch.full((len(features), n), pad, dtype=torch.long)
            for i, f in enumerate(features):
                v = torch.as_tensor(f[k], dtype=torch.long)
                t[i, : v.numel()] = v
            out[k] = t
        return out


@dataclass
class VLPPODataCollator:
    r"""reference :114-126: no padding - every key becomes the LIST of the rows' values, `input_ids` / `attention_mask` as one LongTensor
    per row (VLPPOTrainer.generate left-pads the queries itself).  The model packages add the image tensors."""

    processor: Optional[Any] = None

    def __call__(self, features: List[Dict[str, Any]]) -> Dict[str, Any]:
        batch: Dict[str, Any] = {}
        for key in features[0].keys():
            batch[key] = [torch.as_tensor(f[key], dtype=torch.long) if key in ("input_ids", "attention_mask") else f[key] for f in features]
        return batch


KTO_BATCH_OF_ONE = ("KTO needs per_device_train_batch_size > 1: the KL row of a batch row carries another row's completion, and with one row "
                    "the KL term would be that row's own implied reward")


@dataclass
class VLKTODataCollatorWithPadding:
    r"""KTO rows (`completion_input_ids / _attention_mask / _labels`, `label`, `img_path`) -> a `[chosen ; rejected]`-shaped batch of the
    family's DPO collator: `chosen_*` holds the B main rows, `rejected_*` their KL rows, the image inputs are those of the B rows (the
    pair contract: both halves share prompt and image), `kto_label` [B] uint8 is 1 where the row is desirable.

    The KL row of batch row i is prompt i (and image i) with the completion of row (i - 1) mod B - trl's KTOTrainer shifts the completions
    of a batch by one the same way.  A row's prompt is its leading columns labelled label_pad_token_id, its completion the rest.  The
    prompt does not move: the KL row carries the main row's prompt columns as the tokeniser left them (so both halves of the batch hold
    the same image tokens for the same images), and where prompt + completion exceed max_length the COMPLETION is cut as the tokeniser
    cuts an answer - to max_length - max_prompt_length, or to what the kept prompt leaves of max_length where that is less (at least
    one token).  Labels: label_pad_token_id on the prompt, the completion's own labels behind it."""

    dpo_collator: Any
    max_length: int = 512
    max_prompt_length: int = 128
    label_pad_token_id: int = -100

    def _split(self, row):
        labels = list(row["completion_labels"])
        n = 0
        while n < len(labels) and labels[n] == self.label_pad_token_id:
            n += 1
        return n

    def kl_row(self, row, other) -> Dict[str, Any]:
        """prompt of `row` + completion of `other`, the completion cut to fit, labelled as a tokenised row is"""
        n, k = self._split(row), self._split(other)
        prompt = {f: list(row[f"completion_{f}"][:n]) for f in ("input_ids", "attention_mask")}
        answer = {f: list(other[f"completion_{f}"][k:]) for f in ("input_ids", "attention_mask", "labels")}
        if n + len(answer["input_ids"]) > self.max_length:
            keep = max(1, self.max_length - max(n, self.max_prompt_length))
            answer = {f: v[:keep] for f, v in answer.items()}
        return dict(input_ids=prompt["input_ids"] + answer["input_ids"], attention_mask=prompt["attention_mask"] + answer["attention_mask"],
                    labels=[self.label_pad_token_id] * n + answer["labels"])

    def __call__(self, features: List[Dict[str, Any]]) -> Dict[str, Any]:
        B = len(features)
        if B < 2:
            raise ValueError(KTO_BATCH_OF_ONE)
        rows = []
        for i, f in enumerate(features):
            kl = self.kl_row(f, features[(i - 1) % B])
            row = {f"chosen_{k}": list(f[f"completion_{k}"]) for k in ("input_ids", "attention_mask", "labels")}
            row.update({f"rejected_{k}": v for k, v in kl.items()})
            row["img_path"] = f["img_path"]
            row["label"] = bool(f["label"])
            rows.append(row)
        out = self.dpo_collator(rows)
        out["kto_label"] = torch.tensor([int(r["label"]) for r in rows], dtype=torch.uint8)
        return out
