"""Architecture string -> model package dispatch (mirror of /root/reference/src/vlrlhf/utils/auto_load.py:41-93,
118-139, 190-308, 509-578 for the DPO path)."""
import json
import os
from importlib import import_module

from .. import gptq

MODEL_NICKNAME_MAP = {
    "LlavaForConditionalGeneration": "Llava",
    "LlavaNextForConditionalGeneration": "LlavaNext",
    "QWenLMHeadModel": "QwenVL",
    "InternLMXComposer2ForCausalLM": "InternLMXC2",
    "InstructBlipForConditionalGeneration": "InstructBlip",
    "LlavaForRL": "Llava",
    "LlavaNextForRL": "LlavaNext",
    "QWenLMHeadModel": "QwenVL",
    "QwenVLForRL": "QwenVL",
    "InternLMXC2ForRL": "InternLMXC2",
}
FLASH_ATTN_MODELS = ["LlavaForConditionalGeneration", "LlavaNextForConditionalGeneration", "LlavaForRL"]
IMPLEMENTED = ["Llava", "LlavaNext", "QwenVL", "InternLMXC2"]


def _architecture(model_name_or_path):
    with open(os.path.join(model_name_or_path, "config.json")) as f:
        return json.load(f)["architectures"][0]


def auto_core_mapper(architecture: str):
    nick = MODEL_NICKNAME_MAP[architecture]
    if nick not in IMPLEMENTED:
        raise NotImplementedError(f"{nick}: only {IMPLEMENTED} have an MI355X DPO path so far (SURVEY.md 8f rank 4)")
    return import_module(f".{nick}", "vlrlhf.models").core_mapper


class MyAutoModel:
    @classmethod
    def from_pretrained(cls, model_name_or_path, *args, **kwargs):
        return auto_core_mapper(_architecture(model_name_or_path)).model.from_pretrained(model_name_or_path, *args, **kwargs)


class MyAutoProcessor:
    @classmethod
    def from_pretrained(cls, model_name_or_path, **kwargs):
        return auto_core_mapper(_architecture(model_name_or_path)).processor(model_name_or_path, **kwargs)


class MyAutoDPOCollator:
    def __new__(cls, model_name_or_path, pad_token_id=0, label_pad_token_id=-100, is_encoder_decoder=False, processor=None):
        return auto_core_mapper(_architecture(model_name_or_path)).dpo_collator(pad_token_id, label_pad_token_id,
                                                                                is_encoder_decoder, processor)


class MyAutoDPOTrainer:
    def __new__(cls, model_name_or_path, *args, **kwargs):
        return auto_core_mapper(_architecture(model_name_or_path)).dpo_trainer(*args, **kwargs)


class MyAutoKTOCollator:
    def __new__(cls, model_name_or_path, pad_token_id=0, label_pad_token_id=-100, processor=None, max_length=512, max_prompt_length=128):
        """the family's DPO collator behind the KTO collator: a KTO batch is a `[chosen ; rejected]`-shaped batch of main and KL rows"""
        from ..base.collator import VLKTODataCollatorWithPadding
        nick = MODEL_NICKNAME_MAP[_architecture(model_name_or_path)]
        auto_core_mapper(_architecture(model_name_or_path))      # (refuses the families without an MI355X path)
        dpo = import_module(f".{nick}", "vlrlhf.models").kto_core.dpo_collator(pad_token_id, label_pad_token_id, False, processor)
        return VLKTODataCollatorWithPadding(dpo, max_length=max_length, max_prompt_length=max_prompt_length,
                                            label_pad_token_id=label_pad_token_id)


class MyAutoKTOTrainer:
    def __new__(cls, model_name_or_path, *args, **kwargs):
        nick = MODEL_NICKNAME_MAP[_architecture(model_name_or_path)]
        auto_core_mapper(_architecture(model_name_or_path))
        return import_module(f".{nick}", "vlrlhf.models").kto_core.trainer(*args, **kwargs)


class MyAutoSFTCollator:
    def __new__(cls, model_name_or_path, pad_token_id=0, label_pad_token_id=-100, processor=None):
        return auto_core_mapper(_architecture(model_name_or_path)).sft_collator(pad_token_id, label_pad_token_id, processor)


class MyAutoSFTTrainer:
    def __new__(cls, model_name_or_path, *args, **kwargs):
        return auto_core_mapper(_architecture(model_name_or_path)).sft_trainer(*args, **kwargs)


RM_FAMILIES = ["Llava", "QwenVL"]      # LLaVA-Next's left-padded anyres merge and InternLM-XComposer2's PLoRA rows need their own reward-row rule


def _reward_slot(architecture: str, slot: str):
    nick = MODEL_NICKNAME_MAP[architecture]
    got = getattr(auto_core_mapper(architecture), slot)
    if got is None:
        raise NotImplementedError(f"{nick}: the MI355X reward model covers {RM_FAMILIES} (LLaVA-1.5 and Qwen-VL) only")
    return got


class MyAutoRewardModel:
    @classmethod
    def from_pretrained(cls, model_name_or_path, *args, **kwargs):
        return _reward_slot(_architecture(model_name_or_path), "reward_model").from_pretrained(model_name_or_path, *args, **kwargs)


class MyAutoRMCollator:
    def __new__(cls, model_name_or_path, pad_token_id=0, processor=None):
        return _reward_slot(_architecture(model_name_or_path), "reward_collator")(pad_token_id, processor)


class MyAutoRMTrainer:
    def __new__(cls, model_name_or_path, *args, **kwargs):
        return _reward_slot(_architecture(model_name_or_path), "reward_trainer")(*args, **kwargs)


PPO_FAMILIES = ["Llava", "QwenVL"]      # the families of the reward model: PPO scores its samples with one


def _ppo_slot(architecture: str, slot: str):
    """the PPO record of a model package (`ppo_core`, models/utils.py PPOCore) - not ModelCoreMapper, whose PPO slots stay None"""
    nick = MODEL_NICKNAME_MAP[architecture]
    if nick not in PPO_FAMILIES:
        raise NotImplementedError(f"{nick}: PPO on the MI355X path covers {PPO_FAMILIES} (LLaVA-1.5 and Qwen-VL) only")
    got = getattr(import_module(f".{nick}", "vlrlhf.models").ppo_core, slot)
    if got is None:
        raise NotImplementedError(f"{nick}: the PPO {slot} is not built on the MI355X path yet (the value-head model and the trainer's step are)")
    return got


class MyAutoModelWithValueHead:
    @classmethod
    def from_pretrained(cls, model_name_or_path, *args, **kwargs):
        return _ppo_slot(_architecture(model_name_or_path), "value_model").from_pretrained(model_name_or_path, *args, **kwargs)


class MyAutoPPOTrainer:
    def __new__(cls, model_name_or_path, *args, **kwargs):
        return _ppo_slot(_architecture(model_name_or_path), "trainer")(*args, **kwargs)


class MyAutoPPOCollator:
    def __new__(cls, model_name_or_path, processor=None):
        return _ppo_slot(_architecture(model_name_or_path), "collator")(processor)


GRPO_FAMILIES = ["Llava", "QwenVL"]      # the families whose plain wrapper samples several rows per prompt and has a reward model


def _grpo_slot(architecture: str, slot: str):
    """the GRPO record of a model package (`grpo_core`, models/utils.py GRPOCore)"""
    nick = MODEL_NICKNAME_MAP[architecture]
    if nick not in GRPO_FAMILIES:
        raise NotImplementedError(f"{nick}: GRPO on the MI355X path covers {GRPO_FAMILIES} (LLaVA-1.5 and Qwen-VL) only")
    return getattr(import_module(f".{nick}", "vlrlhf.models").grpo_core, slot)


class MyAutoGRPOTrainer:
    def __new__(cls, model_name_or_path, *args, **kwargs):
        return _grpo_slot(_architecture(model_name_or_path), "trainer")(*args, **kwargs)


class MyAutoGRPOCollator:
    def __new__(cls, model_name_or_path, processor=None):
        return _grpo_slot(_architecture(model_name_or_path), "collator")(processor)


class MyAutoGenerationConfig:
    @classmethod
    def from_pretrained(cls, model_name_or_path):
        """the checkpoint's generation_config.json with the family's defaults filled in by the wrapper's
        prepare_default_generation_kwargs (Qwen-VL: stop_words_ids ...) - a plain attribute bag, which is all `generate` reads.  (The
        reference's ppo.py imports a class of this name that its auto_load does not define.)"""
        from ..eval.utils import read_generation_config
        model_cls = auto_core_mapper(_architecture(model_name_or_path)).model
        gc = read_generation_config(model_name_or_path)
        out = model_cls.prepare_default_generation_kwargs(None, gc)      # (the method reads nothing of the instance)
        return out.get("generation_config", gc)


TOWER_FAMILIES = ["Llava", "LlavaNext"]      # --freeze_vision_tower False: the families whose CLIP tower has a backward (engine._vision_backward)


def auto_load_rlmodel(script_args, training_args, lora_args):
    """-> (model, ref_model=None, lora_config); vision tower frozen unless --freeze_vision_tower False (reference :554-555), which a full
    fine-tune of LLaVA-1.5 / LLaVA-Next honours, LoRA accepts as the no-op it is in the reference, and the other families refuse by
    name.  With use_lora the LoraConfig of
    reference :559-571 is returned as a plain dict (peft itself is not needed: the trainer hands it to
    LlavaForRL.apply_lora).

    q_lora (reference :520-548 loads the checkpoint under GPTQConfig(bits=lora_args.bits, disable_exllama=True)): a checkpoint whose
    config.json carries a GPTQ `quantization_config` loads with its decoder projections PACKED (int4 in HBM, vlrlhf/gptq.py), whether
    or not the flag is given - the reference's from_pretrained does the same.  Packed weights cannot be trained, so such a model needs
    use_lora (ValueError otherwise); q_lora on an unquantised checkpoint is a ValueError too: nothing here quantises, there is no
    calibration set.  --bits other than 4, or a checkpoint of another width, raise NotImplementedError."""
    use_lora = bool(getattr(training_args, "use_lora", False))
    q_lora = use_lora and bool(getattr(lora_args, "q_lora", False))
    with open(os.path.join(script_args.model_name_or_path, "config.json")) as f:
        quant = gptq.parse_quantization_config(json.load(f))      # refuses what the kernels do not take, before anything is loaded
    if q_lora:
        if int(getattr(lora_args, "bits", 4)) != 4:
            raise NotImplementedError(f"--q_lora with --bits {lora_args.bits}: the MI355X kernels unpack 4-bit GPTQ weights only")
        if quant is None:
            raise ValueError(f"--q_lora: {script_args.model_name_or_path} has no quantization_config; q_lora trains adapters over an "
                             "already quantised GPTQ checkpoint (nothing is quantised at load time: there is no calibration set)")
    if quant is not None and not use_lora:
        raise ValueError(f"{script_args.model_name_or_path} is a GPTQ checkpoint: packed int4 weights cannot be trained, "
                         "pass --use_lora True (with --q_lora True)")
    train_tower = not getattr(script_args, "freeze_vision_tower", True)
    if train_tower and use_lora:
        # reference :554-559: freeze_vision_tower() is simply not called, and peft then freezes every base weight - the flag is a no-op
        print("[vlrlhf] --freeze_vision_tower False with --use_lora True: peft freezes every base weight, the vision tower stays frozen",
              flush=True)
        train_tower = False
    if train_tower:
        nick = MODEL_NICKNAME_MAP[_architecture(script_args.model_name_or_path)]
        if nick not in TOWER_FAMILIES:
            # refuse instead of silently training with a frozen tower
            raise NotImplementedError(f"--freeze_vision_tower False: {nick} has no vision-tower backward on the MI355X path; the tower "
                                      f"trains for {TOWER_FAMILIES} (LLaVA-1.5 and LLaVA-Next) only")
        model = MyAutoModel.from_pretrained(script_args.model_name_or_path, train_vision_tower=True)
    else:
        model = MyAutoModel.from_pretrained(script_args.model_name_or_path)
        model.freeze_vision_tower()
    model.config.label_pad_token_id = script_args.label_pad_token_id
    model.config.use_cache = False
    lora_config = None
    if getattr(training_args, "use_lora", False):
        targets = lora_args.lora_target_modules
        if targets in (None, "auto"):
            targets = model.default_lora_target
        elif isinstance(targets, str):
            targets = targets.split(",")
        lora_config = dict(r=lora_args.lora_r, lora_alpha=lora_args.lora_alpha, lora_dropout=lora_args.lora_dropout,
                           target_modules=list(targets), bias=lora_args.lora_bias, task_type="CAUSAL_LM",
                           modules_to_save=lora_args.modules_to_save, seed=int(getattr(training_args, "seed", 0)))
    return model, None, lora_config
