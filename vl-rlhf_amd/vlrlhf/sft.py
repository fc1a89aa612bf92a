"""SFT entry point - mirror of the reference src/vlrlhf/sft.py (ScriptArguments :20-45, LoraArguments :48-64, TrainingArguments :67-76,
main :86-131): the stage that precedes DPO in the reference's pipeline (scripts/sft_*.sh).  One process per GPU; the same HIP engine,
training loop and RCCL reducer as vlrlhf.dpo, with the causal-LM cross-entropy as the loss."""
import os
from dataclasses import dataclass
from typing import Optional

from .dpo import LoraArguments, _parse
from .dpo import TrainingArguments as _DPOTrainingArguments


@dataclass
class ScriptArguments:
    """The arguments for the SFT training script (reference :20-45)."""
    data_path: Optional[str] = None
    data_ratio: Optional[float] = 1.0
    image_root: Optional[str] = None
    dataset_name: Optional[str] = None
    model_name_or_path: Optional[str] = "llava-hf/llava-1.5-7b-hf"
    max_length: Optional[int] = 512
    ignore_bias_buffers: Optional[bool] = False
    label_pad_token_id: Optional[int] = -100
    freeze_vision_tower: bool = True
    merge_peft_model: bool = False
    # not in the reference: shape of the `--dataset_name synthetic_conversations` rows (benchmarks / tests)
    synthetic_rows: int = 64
    synthetic_image_size: int = 336


@dataclass
class TrainingArguments(_DPOTrainingArguments):
    """the fields of vlrlhf.dpo.TrainingArguments with the reference's SFT defaults (:67-76; transformers' learning rate and Adam betas)"""
    learning_rate: float = 5e-5
    adam_beta2: float = 0.999
    adam_epsilon: float = 1e-8
    dataset_num_proc: Optional[int] = 4
    group_name: Optional[str] = "Qwen-VL-Chat-sft"
    run_name: str = "sft"


def main(argv=None):
    from vlrlhf.parallel import init_distributed_from_env
    from vlrlhf.utils.auto_load import MyAutoProcessor, MyAutoSFTCollator, MyAutoSFTTrainer, auto_load_rlmodel
    from vlrlhf.utils.data import DATASET_MAP
    script_args, training_args, lora_args = _parse(ScriptArguments, TrainingArguments, LoraArguments, argv=argv)
    rank, local, world = init_distributed_from_env()
    training_args.local_rank = local
    model, _, lora_config = auto_load_rlmodel(script_args, training_args, lora_args)
    model.engine.gradient_checkpointing = bool(training_args.gradient_checkpointing)
    processor = MyAutoProcessor.from_pretrained(script_args.model_name_or_path)
    processor.train()
    dataset = DATASET_MAP[script_args.dataset_name](script_args)
    # reference :101-105: dataset.train_test_split(test_size=0.005, seed=42) (at least one eval row, as `datasets` rounds up)
    import random
    n_eval = max(1, -(-len(dataset) * 5 // 1000))
    idx = list(range(len(dataset)))
    random.Random(42).shuffle(idx)
    eval_dataset = [dataset[i] for i in idx[:n_eval]]
    # The reference builds train_dataset = the split's train part cut to data_ratio (:103-104) and then hands the trainer
    # `train_dataset=dataset`, the UNSPLIT set (:118): it trains on its own eval rows and data_ratio has no effect.  Fixed here on
    # purpose: the trainer gets the train part.
    train_dataset = [dataset[i] for i in idx[n_eval:]]
    train_dataset = train_dataset[: int(len(train_dataset) * script_args.data_ratio)]
    collator = MyAutoSFTCollator(script_args.model_name_or_path, processor.tokenizer.pad_token_id, script_args.label_pad_token_id,
                                 processor=processor)
    sft_trainer = MyAutoSFTTrainer(
        model_name_or_path=script_args.model_name_or_path, model=model, args=training_args, data_collator=collator,
        train_dataset=train_dataset, eval_dataset=eval_dataset, processor=processor, max_seq_length=script_args.max_length,
        peft_config=lora_config, dataset_num_proc=training_args.dataset_num_proc)
    if world > 1:
        model.engine.make_reducer()           # after the trainer: with peft_config only the adapters are reduced
    sft_trainer.train(resume_from_checkpoint=training_args.resume_from_checkpoint)
    sft_trainer.save_state()
    if rank == 0:
        # reference :126-131: adapters only under LoRA (the PeftSavingCallback does the same for every checkpoint-*: here
        # VLTrainerLoop.save_checkpoint), else the whole model; --merge_peft_model writes the merged model to output_dir/merged
        if training_args.use_lora:
            model.save_adapter(training_args.output_dir, base_model_name_or_path=script_args.model_name_or_path)
        else:
            model.save_pretrained(training_args.output_dir)
        processor.save_pretrained(training_args.output_dir)
        if script_args.merge_peft_model and training_args.use_lora:
            model.save_pretrained(os.path.join(training_args.output_dir, "merged"), state_dict=model.merge_and_unload())
    return sft_trainer


if __name__ == "__main__":
    main()
