"""PPO entry point - mirror of the reference src/vlrlhf/ppo.py (ScriptArguments :27-53, LoraArguments :56-71, PPOConfig :74-125, main
:128-232): the stage after the reward model in the reference's pipeline.  One process, one GPU (VLPPOTrainer refuses more: whitening and
the KL mean are per process in trl); the policy with its value head samples, a separate reward model scores, VLPPOTrainer.step optimises.
LLaVA-1.5 and Qwen-VL (MyAutoModelWithValueHead refuses the other families).

The reference calls build_dataset_from_vlquery_json(local_rank, data_dir, image_root) - a signature its own utils/data.py does not have;
here the builder of this repository is used (`--data_path`, or the reference's `--data_dir`, a JSON list of rows with `query` and `image`),
and `--dataset_name synthetic_queries` makes rows for tests."""
import sys
from dataclasses import dataclass
from typing import Optional

from .base.trainer import PPOConfig as _StepConfig
from .dpo import _parse as _dpo_parse


@dataclass
class ScriptArguments:
    """The arguments for the PPO training script (reference :27-53)."""
    data_dir: Optional[str] = None
    image_root: Optional[str] = None
    model_name_or_path: Optional[str] = "llava-hf/llava-1.5-7b-hf"
    reward_adapter: Optional[str] = None
    reward_adapter_name: Optional[str] = "reward_adapter"
    reward_model_name_or_path: Optional[str] = None
    ignore_bias_buffers: Optional[bool] = False
    freeze_vision_tower: bool = True
    v_head_init_strategy: Optional[str] = "normal"
    v_head_initializer_range: Optional[float] = 0.2
    # not in the reference: the dataset builders of this repository and the synthetic rows of the tests
    dataset_name: Optional[str] = "vlquery_json"
    data_path: Optional[str] = None
    synthetic_rows: int = 8
    synthetic_image_size: int = 336


@dataclass
class LoraArguments:
    """reference :56-71"""
    lora_r: int = 64
    lora_alpha: int = 16
    lora_dropout: float = 0.05
    lora_target_modules: Optional[str] = None
    lora_bias: str = "none"
    q_lora: bool = False
    bits: int = 4
    modules_to_save: Optional[str] = None


@dataclass
class PPOConfig(_StepConfig):
    """the trl 0.8.1 fields the step reads and the reference's additions (vlrlhf.base.trainer.PPOConfig holds both and their rules), plus
    the reference's fields this path accepts and does not act on: the wandb names, the dtype switches (the engine is bf16), fsdp"""
    run_name: Optional[str] = None
    project_name: Optional[str] = "VL-RLHF"
    group_name: Optional[str] = "Qwen-VL-Chat-ppo"
    fp16: bool = False
    bf16: bool = False
    tf32: bool = False
    fsdp: str = ""

    def __post_init__(self):
        super().__post_init__()
        if self.fp16 and self.bf16:
            raise ValueError("You can only use one of fp16 and bf16")


def make_synthetic_query_dataset(script_args):
    """`--dataset_name synthetic_queries`: vlquery-shaped rows {query, image, img_path} with random image tensors, for tests"""
    import torch
    g = torch.Generator().manual_seed(2468)
    words = ["alpha", "beta", "gamma", "delta", "red", "blue", "cat", "dog", "tree", "car", "sky", "left", "right"]
    size = int(script_args.synthetic_image_size)
    rows = []
    for r in range(int(script_args.synthetic_rows)):
        k = int(torch.randint(3, 8, (1,), generator=g))
        q = "What is shown? " + " ".join(words[int(i)] for i in torch.randint(0, len(words), (k,), generator=g))
        rows.append(dict(query=q, image=f"synthetic_{r}", img_path=torch.randn(3, size, size, generator=g)))
    return rows


def lora_config_from_args(model, ppo_config, lora_args):
    """reference :151-161 as a plain dict (VLModelWithValueHead.apply_lora reads it); None without --use_lora"""
    if not ppo_config.use_lora:
        return None
    if lora_args.q_lora:
        raise NotImplementedError("--q_lora: PPO over GPTQ int4 base weights is not supported on the MI355X path")
    targets = lora_args.lora_target_modules
    if targets in (None, "auto"):
        targets = model.pretrained_model.default_lora_target
    elif isinstance(targets, str):
        targets = targets.split(",")
    mts = lora_args.modules_to_save
    return dict(r=lora_args.lora_r, lora_alpha=lora_args.lora_alpha, lora_dropout=lora_args.lora_dropout, target_modules=list(targets),
                bias=lora_args.lora_bias, task_type="CAUSAL_LM", modules_to_save=mts.split(",") if isinstance(mts, str) else mts,
                seed=int(ppo_config.seed))


def generation_config_for(model_name_or_path, ppo_config):
    """reference :207-214: the checkpoint's generation config with top_p = 1.0 and the length limit the PPO config names - max_new_tokens
    as given, or max_length with max_new_tokens cleared (generate prefers max_new_tokens when both are set)"""
    from .utils.auto_load import MyAutoGenerationConfig
    gc = MyAutoGenerationConfig.from_pretrained(model_name_or_path)
    gc.top_p = 1.0
    if ppo_config.max_new_tokens is not None:
        gc.max_new_tokens = ppo_config.max_new_tokens
    if ppo_config.max_length is not None:
        gc.max_length = ppo_config.max_length
        gc.max_new_tokens = None
    return gc


def _parse(argv=None):
    """the three dataclasses from the command line; unknown arguments are named on stderr and ignored, as vlrlhf.dpo does"""
    import contextlib
    import io
    err = io.StringIO()
    try:
        with contextlib.redirect_stderr(err):
            return _dpo_parse(ScriptArguments, PPOConfig, LoraArguments, argv=argv)
    finally:      # the shared parser signs its warning with the DPO script's name
        msg = err.getvalue().replace("[vlrlhf.dpo]", "[vlrlhf.ppo]")
        if msg:
            print(msg, end="", file=sys.stderr, flush=True)


def main(argv=None):
    from .utils.auto_load import MyAutoModelWithValueHead, MyAutoPPOCollator, MyAutoPPOTrainer, MyAutoProcessor, MyAutoRewardModel
    from .utils.data import DATASET_MAP
    script_args, ppo_config, lora_args = _parse(argv)
    if not script_args.freeze_vision_tower:
        raise NotImplementedError("--freeze_vision_tower False: the MI355X path has no vision-tower backward")
    if script_args.reward_adapter is not None and script_args.reward_model_name_or_path is not None:
        raise ValueError("You can only use one of reward_adapter and reward_model")
    if script_args.reward_adapter is not None:
        raise NotImplementedError("--reward_adapter: a reward adapter on the policy's base is not built on the MI355X path; pass "
                                  "--reward_model_name_or_path (a directory written by vlrlhf.reward_modeling)")
    if ppo_config.use_value_adapter:
        raise NotImplementedError("--use_value_adapter: a value adapter on a shared base is not built on the MI355X path")
    if script_args.reward_model_name_or_path is None:
        raise ValueError("PPO needs a reward model: pass --reward_model_name_or_path")
    if script_args.data_path is None:
        script_args.data_path = script_args.data_dir
    reward_model = MyAutoRewardModel.from_pretrained(script_args.reward_model_name_or_path)
    reward_model.eval()
    model = MyAutoModelWithValueHead.from_pretrained(
        script_args.model_name_or_path, v_head_init_strategy=script_args.v_head_init_strategy,
        v_head_initializer_range=script_args.v_head_initializer_range, seed=ppo_config.seed)
    model.pretrained_model.freeze_vision_tower()
    model.pretrained_model.config.use_cache = False
    if hasattr(model.pretrained_model, "enable_kv_cache"):      # Qwen-VL samples from the KV cache only when asked to: PPO asks
        model.pretrained_model.enable_kv_cache()
    if ppo_config.gradient_checkpointing:
        model.gradient_checkpointing_enable()
    lora_config = lora_config_from_args(model, ppo_config, lora_args)
    if lora_config is not None:
        model.apply_lora(lora_config)
    processor = MyAutoProcessor.from_pretrained(script_args.model_name_or_path)
    processor.train()
    builders = dict(DATASET_MAP, synthetic_queries=make_synthetic_query_dataset)
    dataset = builders[script_args.dataset_name](script_args)
    generation_config = generation_config_for(script_args.model_name_or_path, ppo_config)
    data_collator = MyAutoPPOCollator(script_args.model_name_or_path, processor=processor)
    ppo_trainer = MyAutoPPOTrainer(
        script_args.model_name_or_path, config=ppo_config, model=model, ref_model=None, reward_model=reward_model, processor=processor,
        dataset=dataset, data_collator=data_collator, generation_kwargs={"generation_config": generation_config, "use_cache": True})
    ppo_trainer.train(resume_from_checkpoint=ppo_config.resume_from_checkpoint)
    if ppo_config.output_dir:
        # reference safe_save_model_for_ppo_trainer: the adapter + pytorch_model.bin (the value head) under LoRA, else the whole model
        if ppo_config.use_lora:
            model.save_adapter(ppo_config.output_dir, base_model_name_or_path=script_args.model_name_or_path)
        else:
            model.save_pretrained(ppo_config.output_dir)
        processor.save_pretrained(ppo_config.output_dir)
    return ppo_trainer


if __name__ == "__main__":
    main()
