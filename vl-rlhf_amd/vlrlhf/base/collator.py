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

