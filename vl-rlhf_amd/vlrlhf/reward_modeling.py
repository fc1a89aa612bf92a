"""Reward-model entry point - mirror of the reference src/vlrlhf/reward_modeling.py (ScriptArguments :18-47, LoraArguments :50-65,
TrainingArguments :68-74, main :86-178): the stage between SFT and PPO / DPO in the reference's pipeline.  One process per GPU; the
same HIP engine, training loop and RCCL reducer as vlrlhf.dpo, with the pair loss -logsigmoid(r_chosen - r_rejected) on the rewards
of `rm_head`.  LLaVA-1.5 and Qwen-VL (MyAutoRewardModel refuses the other families).

The reference calls make_vlfeedback_paired_dataset(local_rank, data_dir, score_margin) - a signature its own utils/data.py no longer
has; here the dataset builders of this repository are used (`--dataset_name`, default vlfeedback_paired, `--data_path` or the
reference's `--data_dir`)."""
from dataclasses import dataclass
from typing import Optional

from .dpo import _parse
from .dpo import LoraArguments as _DPOLoraArguments
from .dpo import TrainingArguments as _DPOTrainingArguments


@dataclass
class ScriptArguments:
    """The arguments for the RM training script (reference :18-47)."""
    score_margin: Optional[float] = -1
    data_dir: Optional[str] = None
    model_name_or_path: Optional[str] = "llava-hf/llava-1.5-7b-hf"
    max_length: Optional[int] = 512
    ignore_bias_buffers: Optional[bool] = False
    freeze_vision_tower: bool = True
    # not in the reference: the dataset builders of this repository (vlrlhf.utils.data.DATASET_MAP) and the synthetic rows of the tests
    dataset_name: Optional[str] = "vlfeedback_paired"
    data_path: Optional[str] = None
    image_root: Optional[str] = None
    synthetic_rows: int = 64
    synthetic_image_size: int = 336


@dataclass
class LoraArguments(_DPOLoraArguments):
    """reference :50-65: the DPO script's fields with modules_to_save defaulting to the reward head"""
    modules_to_save: Optional[str] = "rm_head"


@dataclass
class TrainingArguments(_DPOTrainingArguments):
    """the fields of vlrlhf.dpo.TrainingArguments with the reference's RM defaults (:68-74; transformers' learning rate and Adam betas)"""
    learning_rate: float = 5e-5
    adam_beta2: float = 0.999
    adam_epsilon: float = 1e-8
    group_name: Optional[str] = "Qwen-VL-Chat-rm"
    run_name: str = "rm"


def lora_config_from_args(model, training_args, lora_args):
    """reference :129-139 as a plain dict (VLRewardModel.apply_lora reads it); None without --use_lora"""
    if not getattr(training_args, "use_lora", False):
        return None
    if getattr(lora_args, "q_lora", False):
        raise NotImplementedError("--q_lora: reward modelling over GPTQ int4 base weights is not supported on the MI355X path")
    targets = lora_args.lora_target_modules
    if targets in (None, "auto"):
        targets = model.base_model.default_lora_target
    elif isinstance(targets, str):
        targets = targets.split(",")
    mts = lora_args.modules_to_save
    return dict(r=lora_args.lora_r, lora_alpha=lora_args.lora_alpha, lora_dropout=lora_args.lora_dropout, target_modules=list(targets),
                bias=lora_args.lora_bias, task_type="CAUSAL_LM", modules_to_save=mts.split(",") if isinstance(mts, str) else mts,
                seed=int(getattr(training_args, "seed", 0)))


def main(argv=None):
    from vlrlhf.parallel import init_distributed_from_env
    from vlrlhf.utils.auto_load import MyAutoProcessor, MyAutoRewardModel, MyAutoRMCollator, MyAutoRMTrainer
    from vlrlhf.utils.data import DATASET_MAP
    script_args, training_args, lora_args = _parse(ScriptArguments, TrainingArguments, LoraArguments, argv=argv)
    rank, local, world = init_distributed_from_env()
    training_args.local_rank = local
    if not script_args.freeze_vision_tower:
        raise NotImplementedError("--freeze_vision_tower False: the MI355X path has no vision-tower backward")
    if script_args.data_path is None:
        script_args.data_path = script_args.data_dir
    model = MyAutoRewardModel.from_pretrained(script_args.model_name_or_path, seed=training_args.seed)
    model.base_model.freeze_vision_tower()
    model.config.use_cache = False
    if training_args.gradient_checkpointing:
        model.gradient_checkpointing_enable()
    lora_config = lora_config_from_args(model, training_args, lora_args)
    processor = MyAutoProcessor.from_pretrained(script_args.model_name_or_path)
    processor.train()
    dataset = DATASET_MAP[script_args.dataset_name](script_args)
    # reference :153: dataset.train_test_split(test_size=0.005, seed=42) (at least one eval row, as `datasets` rounds up)
    import random
    n_eval = max(1, -(-len(dataset) * 5 // 1000))
    idx = list(range(len(dataset)))
    random.Random(42).shuffle(idx)
    eval_dataset = [dataset[i] for i in idx[:n_eval]]
    train_dataset = [dataset[i] for i in idx[n_eval:]]
    data_collator = MyAutoRMCollator(script_args.model_name_or_path, pad_token_id=processor.tokenizer.pad_token_id, processor=processor)
    rm_trainer = MyAutoRMTrainer(
        script_args.model_name_or_path, model=model, args=training_args, train_dataset=train_dataset, eval_dataset=eval_dataset,
        processor=processor, max_length=script_args.max_length, data_collator=data_collator, peft_config=lora_config)
    if world > 1:
        model.engine.make_reducer()           # after the trainer: with peft_config only the adapters and the head are reduced
    rm_trainer.train(resume_from_checkpoint=training_args.resume_from_checkpoint)
    rm_trainer.save_state()
    if rank == 0:
        # reference :177: safe_save_model_for_hf_trainer - the adapter (and rm_head.bin) under LoRA, else the whole model + rm_head.bin
        if training_args.use_lora:
            model.save_adapter(training_args.output_dir, base_model_name_or_path=script_args.model_name_or_path)
        else:
            model.save_pretrained(training_args.output_dir)
        processor.save_pretrained(training_args.output_dir)
    return rm_trainer


if __name__ == "__main__":
    main()
