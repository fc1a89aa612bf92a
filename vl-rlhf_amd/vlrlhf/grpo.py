"""GRPO entry point, on the pattern of vlrlhf/ppo.py: Group Relative Policy Optimization next to PPO.  One process, one GPU
(VLGRPOTrainer refuses more: it has never been run); the policy is the plain family wrapper - no value head - which samples
num_generations responses per query from one call of its generate; a separate reward model scores them, or a `reward_fn(queries_text,
responses_text) -> list of floats` handed to main() (rule-based rewards); VLGRPOTrainer.step optimises.  LLaVA-1.5 and Qwen-VL
(MyAutoGRPOTrainer refuses the other families).

The dataset builders are those of vlrlhf/ppo.py (`--data_path`, or `--data_dir`, a JSON list of rows with `query` and `image`);
`--dataset_name synthetic_queries` makes rows for tests."""
import sys
from dataclasses import dataclass
from typing import Optional

from .base.trainer import GRPOConfig as _StepConfig
from .dpo import _parse as _dpo_parse
from .ppo import LoraArguments, make_synthetic_query_dataset  # noqa: F401  (the same adapter arguments and synthetic rows as PPO)


@dataclass
class ScriptArguments:
    """The arguments for the GRPO training script (the PPO script's, without the value head's)."""
    data_dir: Optional[str] = None
    image_root: Optional[str] = None
    model_name_or_path: Optional[str] = "llava-hf/llava-1.5-7b-hf"
    reward_model_name_or_path: Optional[str] = None
    ignore_bias_buffers: Optional[bool] = False
    freeze_vision_tower: bool = True
    dataset_name: Optional[str] = "vlquery_json"
    data_path: Optional[str] = None
    synthetic_rows: int = 8
    synthetic_image_size: int = 336


@dataclass
class GRPOConfig(_StepConfig):
    """the fields the step reads (vlrlhf.base.trainer.GRPOConfig holds them and their rules), plus the fields of the PPO script this path
    accepts and does not act on: the wandb names, the dtype switches (the engine is bf16), fsdp"""
    run_name: Optional[str] = None
    project_name: Optional[str] = "VL-RLHF"
    group_name: Optional[str] = "llava-grpo"
    fp16: bool = False
    bf16: bool = False
    tf32: bool = False
    fsdp: str = ""

    def __post_init__(self):
        super().__post_init__()
        if self.fp16 and self.bf16:
            raise ValueError("You can only use one of fp16 and bf16")


def lora_config_from_args(model, grpo_config, lora_args):
    """the adapter arguments as the plain dict LlavaForRL.apply_lora reads; None without --use_lora"""
    if not grpo_config.use_lora:
        return None
    if lora_args.q_lora:
        raise NotImplementedError("--q_lora: GRPO over GPTQ int4 base weights is not supported on the MI355X path")
    targets = lora_args.lora_target_modules
    if targets in (None, "auto"):
        targets = model.default_lora_target
    elif isinstance(targets, str):
        targets = targets.split(",")
    return dict(r=lora_args.lora_r, lora_alpha=lora_args.lora_alpha, lora_dropout=lora_args.lora_dropout, target_modules=list(targets),
                bias=lora_args.lora_bias, task_type="CAUSAL_LM", modules_to_save=lora_args.modules_to_save, seed=int(grpo_config.seed))


def generation_config_for(model_name_or_path, grpo_config):
    """the checkpoint's generation config with top_p = 1.0 and the config's max_new_tokens; VLGRPOTrainer.generate adds do_sample and
    num_return_sequences"""
    from .utils.auto_load import MyAutoGenerationConfig
    gc = MyAutoGenerationConfig.from_pretrained(model_name_or_path)
    gc.top_p = 1.0
    if grpo_config.max_new_tokens is not None:
        gc.max_new_tokens = grpo_config.max_new_tokens
    return gc


def _parse(argv=None):
    """the three dataclasses from the command line; unknown arguments are named on stderr and ignored, as vlrlhf.dpo does"""
    import contextlib
    import io
    err = io.StringIO()
    try:
        with contextlib.redirect_stderr(err):
            return _dpo_parse(ScriptArguments, GRPOConfig, LoraArguments, argv=argv)
    finally:      # the shared parser signs its warning with the DPO script's name
        msg = err.getvalue().replace("[vlrlhf.dpo]", "[vlrlhf.grpo]")
        if msg:
            print(msg, end="", file=sys.stderr, flush=True)


def main(argv=None, reward_fn=None):
    """-> the trainer, after train().  `reward_fn(queries_text, responses_text) -> list of floats` scores in place of a reward model."""
    from .utils.auto_load import MyAutoGRPOCollator, MyAutoGRPOTrainer, MyAutoModel, MyAutoProcessor, MyAutoRewardModel, _architecture, _grpo_slot
    from .utils.data import DATASET_MAP
    script_args, grpo_config, lora_args = _parse(argv)
    if not script_args.freeze_vision_tower:
        raise NotImplementedError("--freeze_vision_tower False: the MI355X path has no vision-tower backward")
    if grpo_config.use_lora and lora_args.q_lora:
        raise NotImplementedError("--q_lora: GRPO over GPTQ int4 base weights is not supported on the MI355X path")
    if int(grpo_config.world_size or 1) > 1:
        raise NotImplementedError("GRPO on more than one GPU has never been run on the MI355X path")
    if script_args.reward_model_name_or_path is not None and reward_fn is not None:
        raise ValueError("You can only use one of --reward_model_name_or_path and reward_fn")
    if script_args.reward_model_name_or_path is None and reward_fn is None:
        raise ValueError("GRPO needs a reward source: pass --reward_model_name_or_path, or a reward_fn to main()")
    if script_args.data_path is None:
        script_args.data_path = script_args.data_dir
    _grpo_slot(_architecture(script_args.model_name_or_path), "trainer")      # a family outside GRPO_FAMILIES is refused before anything is loaded
    reward_model = None
    if script_args.reward_model_name_or_path is not None:
        reward_model = MyAutoRewardModel.from_pretrained(script_args.reward_model_name_or_path)
        reward_model.eval()
    model = MyAutoModel.from_pretrained(script_args.model_name_or_path)
    if model.is_packed:
        raise NotImplementedError("GRPO over GPTQ int4 base weights (q_lora) is not supported on the MI355X path")
    model.freeze_vision_tower()
    model.config.use_cache = False
    if hasattr(model, "enable_kv_cache"):      # Qwen-VL samples from the KV cache only when asked to: GRPO asks
        model.enable_kv_cache()
    if grpo_config.gradient_checkpointing:
        model.gradient_checkpointing_enable()
    lora_config = lora_config_from_args(model, grpo_config, lora_args)
    if lora_config is not None:
        model.apply_lora(lora_config)
    processor = MyAutoProcessor.from_pretrained(script_args.model_name_or_path)
    processor.train()
    builders = dict(DATASET_MAP, synthetic_queries=make_synthetic_query_dataset)
    dataset = builders[script_args.dataset_name](script_args)
    generation_config = generation_config_for(script_args.model_name_or_path, grpo_config)
    data_collator = MyAutoGRPOCollator(script_args.model_name_or_path, processor=processor)
    trainer = MyAutoGRPOTrainer(
        script_args.model_name_or_path, config=grpo_config, model=model, ref_model=None, reward_model=reward_model, processor=processor,
        dataset=dataset, data_collator=data_collator, generation_kwargs={"generation_config": generation_config, "use_cache": True},
        reward_fn=reward_fn)
    trainer.train(resume_from_checkpoint=grpo_config.resume_from_checkpoint)
    if grpo_config.output_dir:
        if grpo_config.use_lora:
            model.save_adapter(grpo_config.output_dir, base_model_name_or_path=script_args.model_name_or_path)
        else:
            model.save_pretrained(grpo_config.output_dir)
        processor.save_pretrained(grpo_config.output_dir)
    return trainer


if __name__ == "__main__":
    main()
