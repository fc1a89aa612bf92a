"""Per-model registry record (mirror of /root/reference/src/vlrlhf/models/utils.py:18-31).  The DPO and SFT slots are filled by every
model package, the reward slots by LLaVA-1.5 and Qwen-VL; the PPO / value slots stay in the record so a reference user finds the same
twelve fields, and are None.

PPO is registered through a record of its own, `ppo_core` (PPOCore: value model, collator, trainer), exported by the packages that cover it
(LLaVA-1.5, Qwen-VL) and resolved by utils/auto_load.py (PPO_FAMILIES, MyAutoModelWithValueHead, MyAutoPPOCollator, MyAutoPPOTrainer):
auto_core_mapper hands a ModelCoreMapper out for all four families, and callers read a filled slot as "this family has the stage"."""
from dataclasses import dataclass
from typing import Any


@dataclass
class ModelCoreMapper:
    model: Any
    processor: Any
    dpo_collator: Any
    dpo_trainer: Any
    reward_model: Any = None
    value_model: Any = None
    reward_collator: Any = None
    reward_trainer: Any = None
    sft_collator: Any = None
    sft_trainer: Any = None
    ppo_collator: Any = None
    ppo_trainer: Any = None


@dataclass
class PPOCore:
    value_model: Any
    collator: Any = None
    trainer: Any = None


@dataclass
class GRPOCore:
    """GRPO's record (`grpo_core`, resolved by utils/auto_load.py GRPO_FAMILIES / MyAutoGRPOTrainer): the policy is the plain wrapper"""
    model: Any
    collator: Any = None
    trainer: Any = None


@dataclass
class KTOCore:
    """KTO's record (`kto_core`, resolved by utils/auto_load.py MyAutoKTOTrainer / MyAutoKTOCollator), exported by every package that has
    a DPO trainer: the rows are collated by the family's DPO collator behind base/collator.py VLKTODataCollatorWithPadding"""
    dpo_collator: Any
    trainer: Any
