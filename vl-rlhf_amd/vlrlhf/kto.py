"""KTO entry point: Kahneman-Tversky Optimization on UNPAIRED feedback (one prompt, one completion, one thumbs-up or thumbs-down per
row) - what trl's KTOTrainer does, where the reference's scripts/kto_*.sh run the paired stand-in (`--loss_type kto_pair` of dpo.py).
Modelled on vlrlhf/dpo.py: the same script and LoRA arguments, KTOConfig (base/trainer.py) for the training arguments plus beta,
desirable_weight and undesirable_weight.  One process, one GPU: more ranks are refused by name."""
import os
from dataclasses import dataclass
from typing import Optional

from .dpo import LoraArguments, _parse


@dataclass
class ScriptArguments:
    data_path: Optional[str] = None
    data_ratio: Optional[float] = 1.0
    image_root: Optional[str] = None
    dataset_name: Optional[str] = "vlfeedback_unpaired"
    score_margin: Optional[float] = -1
    model_name_or_path: Optional[str] = "llava-hf/llava-1.5-7b-hf"
    label_pad_token_id: Optional[int] = -100
    freeze_vision_tower: bool = True
    reference_free: bool = False
    # shape of the `--dataset_name synthetic_unpaired` rows (benchmarks / tests; no network for the hub datasets)
    synthetic_rows: int = 64
    synthetic_image_size: int = 336


def check_arguments(script_args, training_args, lora_args):
    """what KTO refuses, by name and before a checkpoint is read (VLKTOTrainer refuses the same on the objects it is handed)"""
    world = int(os.environ.get("WORLD_SIZE", "1") or 1)
    if world > 1:
        raise NotImplementedError(f"KTO on more than one GPU (WORLD_SIZE={world}): trl averages kl across the ranks, and that has never "
                                  "been run on the MI355X path")
    if training_args.precompute_ref_log_probs:
        raise NotImplementedError("--precompute_ref_log_probs: the KL rows change with the batch's composition, and the pre-pass that "
                                  "would store them per batch is not built")
    if script_args.reference_free:
        raise NotImplementedError("--reference_free: KTO's rewards and its KL baseline are log-ratios against a reference model")
    if training_args.use_lora and lora_args.q_lora:
        raise NotImplementedError("--q_lora: KTO over a packed GPTQ base has never been run on the MI355X path")
    if not script_args.freeze_vision_tower:
        raise NotImplementedError("--freeze_vision_tower False: KTO's two policy passes would both need the tower's backward state; the "
                                  "tower stays frozen on this path")
    if int(training_args.per_device_train_batch_size) < 2:
        from .base.collator import KTO_BATCH_OF_ONE
        raise ValueError(KTO_BATCH_OF_ONE)


def parse_args(argv=None):
    from .base.trainer import KTOConfig
    return _parse(ScriptArguments, KTOConfig, LoraArguments, argv=argv)


def main(argv=None):
    from vlrlhf.parallel import init_distributed_from_env
    from vlrlhf.utils.auto_load import MyAutoKTOCollator, MyAutoKTOTrainer, MyAutoProcessor, auto_load_rlmodel
    from vlrlhf.utils.data import DATASET_MAP
    script_args, training_args, lora_args = parse_args(argv)
    check_arguments(script_args, training_args, lora_args)
    rank, local, world = init_distributed_from_env()
    training_args.local_rank = local
    model, ref_model, lora_config = auto_load_rlmodel(script_args, training_args, lora_args)
    model.engine.gradient_checkpointing = bool(training_args.gradient_checkpointing)
    processor = MyAutoProcessor.from_pretrained(script_args.model_name_or_path)
    processor.train()
    dataset = DATASET_MAP[script_args.dataset_name](script_args)
    n_eval = max(2, int(len(dataset) * 0.005))      # (a KTO batch needs two rows)
    import random
    idx = list(range(len(dataset)))
    random.Random(42).shuffle(idx)
    eval_dataset = [dataset[i] for i in idx[:n_eval]]
    train_dataset = [dataset[i] for i in idx[n_eval:]]
    train_dataset = train_dataset[: int(len(train_dataset) * script_args.data_ratio)]
    data_collator = MyAutoKTOCollator(script_args.model_name_or_path, pad_token_id=processor.tokenizer.pad_token_id,
                                      label_pad_token_id=script_args.label_pad_token_id, processor=processor,
                                      max_length=training_args.max_length, max_prompt_length=training_args.max_prompt_length)
    trainer = MyAutoKTOTrainer(script_args.model_name_or_path, model=model, ref_model=ref_model, args=training_args,
                               train_dataset=train_dataset, eval_dataset=eval_dataset, processor=processor, data_collator=data_collator,
                               peft_config=lora_config, label_pad_token_id=script_args.label_pad_token_id,
                               dataset_num_proc=training_args.dataset_num_proc)
    trainer.train(resume_from_checkpoint=training_args.resume_from_checkpoint)
    trainer.save_state()
    if rank == 0:
        if training_args.use_lora:
            model.save_adapter(training_args.output_dir, base_model_name_or_path=script_args.model_name_or_path)
        else:
            model.save_pretrained(training_args.output_dir)
        processor.save_pretrained(training_args.output_dir)
    return trainer


if __name__ == "__main__":
    main()
