"""VLDPOTrainer, VLSFTTrainer and VLRMTrainer for MI355X - mirror of /root/reference/src/vlrlhf/base/trainer.py:33-360 plus the parts of
trl==0.8.1 `DPOTrainer` and transformers `Trainer` the reference inherits on the DPO path (not vendored there:
constructor bookkeeping, tokenize_row / build_tokenized_answer, concatenated_inputs, compute_loss /
get_batch_loss_metrics, the step loop, clip + AdamW + cosine schedule).

Same names, argument order and error behaviour; the arithmetic (model forward/backward, log-probs, loss, optimizer)
runs in libvlr_hip.so through `vlrlhf.engine` - there is no PyTorch/CPU fallback.  What is deliberately NOT
reproduced: the per-micro-step `torch.cuda.empty_cache(); gc.collect()` (reference :306-307), ZeRO/DeepSpeed, wandb.
"""
import contextlib
import copy
import dataclasses
import math
import os
import random
from collections import defaultdict
from contextlib import nullcontext
from typing import Any, Callable, Dict, List, Literal, Optional, Tuple, Union

import torch
import torch.nn as nn

from .. import _hip
from ..utils.common import pad_to_length
from ..utils.diff_lib import ddpo_shared_mask

LOSS_TYPE_IDS = {"sigmoid": 0, "ddpo": 0, "hinge": 1, "ipo": 2, "kto_pair": 3}


# ----------------------------------------------------------------------------------------------------------
# autograd boundary: three coarse Functions, each a thin shell around C-ABI calls
# ----------------------------------------------------------------------------------------------------------
class _TensorLogpsFn(torch.autograd.Function):
    """get_batch_logps on a MATERIALISED logits tensor [Bn,S,V] (the reference's A4 op): shift, log-softmax pick,
    masked sum - HIP kernels vlr_build_rows / vlr_logp_rows / vlr_seq_sum, backward vlr_dlogits_rows."""

    @staticmethod
    def forward(ctx, logits, labels, shared_mask, average, label_pad):
        Bn, S, V = logits.shape
        dev = logits.device
        lg = logits.detach().float().contiguous().view(Bn * S, V)
        rows = torch.empty(Bn * S, dtype=torch.int32, device=dev)
        tgt = torch.empty(Bn * S, dtype=torch.int32, device=dev)
        seq_off = torch.empty(Bn + 1, dtype=torch.int32, device=dev)
        sm = shared_mask.to(device=dev, dtype=torch.uint8).contiguous() if shared_mask is not None else None
        _hip.call("vlr_build_rows", labels.to(dev).contiguous(), sm, Bn, S, label_pad, rows, tgt, seq_off)
        R = int(seq_off[-1])
        out = torch.zeros(Bn, dtype=torch.float32, device=dev)
        tok = torch.empty(max(R, 1), dtype=torch.float32, device=dev)
        lse = torch.empty(max(R, 1), dtype=torch.float32, device=dev)
        if R:
            _hip.call("vlr_logp_rows", lg, rows, tgt, R, V, V, tok, lse)
            _hip.call("vlr_seq_sum", tok, seq_off, Bn, int(average), out)
        ctx.save_for_backward(lg, rows, tgt, seq_off, lse)
        ctx.meta = (Bn, S, V, R, int(average), logits.dtype)
        return out

    @staticmethod
    def backward(ctx, dlogps):
        lg, rows, tgt, seq_off, lse = ctx.saved_tensors
        Bn, S, V, R, average, dtype = ctx.meta
        grad = torch.zeros(Bn * S, V, dtype=dtype, device=lg.device)
        if R:
            compact = lg[rows[:R].long()].contiguous()
            dl = torch.empty(R, V, dtype=torch.bfloat16, device=lg.device)
            _hip.call("vlr_dlogits_rows", compact, tgt, lse, seq_off, Bn, dlogps.float().contiguous(), average, R, V, V, dl, V)
            grad[rows[:R].long()] = dl.to(dtype)
        return grad.view(Bn, S, V), None, None, None, None


class _DpoLossFn(torch.autograd.Function):
    """VLDPOTrainer.dpo_loss forward + backward in one HIP kernel (vlr_dpo_loss)."""

    @staticmethod
    def forward(ctx, pc, pr, rc, rr, beta, label_smoothing, loss_type_id, reference_free):
        n = pc.shape[0]
        dev = pc.device
        a = [t.detach().float().contiguous() for t in (pc, pr, rc, rr)]
        nl = 2 * n if loss_type_id == 3 else n
        losses = torch.empty(nl, dtype=torch.float32, device=dev)
        cr, rw, dpc, dpr = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(4))
        mean = torch.empty(1, dtype=torch.float32, device=dev)
        _hip.call("vlr_dpo_loss", a[0], a[1], a[2], a[3], n, float(beta), float(label_smoothing), int(loss_type_id),
                  int(reference_free), losses, cr, rw, dpc, dpr, mean, None)
        ctx.save_for_backward(*a)
        ctx.meta = (n, float(beta), float(label_smoothing), int(loss_type_id), int(reference_free))
        ctx.mark_non_differentiable(cr, rw)
        return losses, cr, rw

    @staticmethod
    def backward(ctx, g_losses, g_cr, g_rw):
        a = ctx.saved_tensors
        n, beta, ls, lt, rf = ctx.meta
        dev = a[0].device
        nl = 2 * n if lt == 3 else n
        scratch = [torch.empty(max(nl, n), dtype=torch.float32, device=dev) for _ in range(3)]
        dpc, dpr = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
        mean = torch.empty(1, dtype=torch.float32, device=dev)
        _hip.call("vlr_dpo_loss", a[0], a[1], a[2], a[3], n, beta, ls, lt, rf, scratch[0], scratch[1], scratch[2], dpc, dpr,
                  mean, g_losses.float().contiguous())
        return dpc, dpr, None, None, None, None, None, None


class VLTrainerLoop:
    """The step loop shared by VLDPOTrainer and VLSFTTrainer - what both inherit from transformers.Trainer in the reference: gradient
    accumulation, clip + AdamW + the lr schedule (engine.optimizer_step), checkpoint / resume, evaluate, logging and the RCCL reducer.
    A subclass provides `compute_loss(model, inputs)`, `prediction_step(model, inputs)` and the attributes model / args / train_dataset /
    eval_dataset / data_collator / accelerator / state / log_history / callbacks / is_peft_model / _stored_metrics."""

    # ------------------------------------------------------------------------------------------ NEFTune
    neftune_noise_alpha = None

    def _init_neftune(self, model, args, alpha=None):
        """transformers Trainer.__init__ (`self.neftune_noise_alpha = args.neftune_noise_alpha`) / trl SFTTrainer (the constructor
        argument wins): remembers alpha; a model that cannot apply the noise (no HIP engine behind it) is refused here, not at step 1."""
        if alpha is None:
            alpha = getattr(args, "neftune_noise_alpha", None)
        if alpha is not None and not hasattr(getattr(model, "engine", None), "set_neftune"):
            raise NotImplementedError("neftune_noise_alpha (NEFTune embedding noise) needs a model wrapper on the HIP engine "
                                      "(engine.set_neftune); this one has none")
        self.neftune_noise_alpha = None if alpha is None else float(alpha)

    def _activate_neftune(self):
        """transformers Trainer._activate_neftune: noise on the input embeddings of the training passes from here on.  Key = args.seed
        (low word) and the data-parallel rank (high word); the engine's call counter goes on from where it stands (resume)."""
        if self.neftune_noise_alpha is not None:
            seed = getattr(self.args, "seed", None)
            self.model.engine.set_neftune(self.neftune_noise_alpha, seed=42 if seed is None else int(seed), rank=_rank())

    def _deactivate_neftune(self):
        """transformers Trainer._deactivate_neftune (end of train()): what runs after training sees clean embeddings"""
        if self.neftune_noise_alpha is not None:
            self.model.engine.set_neftune(None)

    # hooks of the loop a subclass may fill (VLDPOTrainer: the reference pre-pass and pipelining, the sampled eval table)
    def _before_train(self):
        self._activate_neftune()

    def prefetch_reference(self, inputs):
        return inputs

    def _before_evaluate(self, ds, explicit: bool):
        pass

    def _evaluate_samples(self, rows, bs):
        pass

    def store_metrics(self, metrics, train_eval="train"):
        for k, v in metrics.items():
            self._stored_metrics[train_eval][k].append(v)

    def log(self, logs: Dict[str, float]):
        """trl DPOTrainer.log + HF Trainer.log: the stored metrics are averaged over the micro-steps since the last log and -
        like the loss HF reports (`_nested_gather(tr_loss).mean()`) - over the data-parallel ranks, with ONE all-reduce of
        the <= 9 scalars.  Every rank must call log() at the same steps (they do: same step counter)."""
        from ..parallel import all_reduce_mean_scalars
        train_eval = "train" if "loss" in logs else "eval"
        keys, vals = [], []
        for k, v in self._stored_metrics[train_eval].items():
            keys.append(k)
            vals.append(torch.stack([torch.as_tensor(x, dtype=torch.float32, device=self.accelerator.device) for x in v]).mean())
        for k in ("loss", "eval_loss"):
            if k in logs:
                keys.append(k)
                vals.append(float(logs[k]))
        self._stored_metrics[train_eval].clear()
        if keys:
            logs.update(zip(keys, all_reduce_mean_scalars(vals, device=self.accelerator.device if _world() > 1 and _backend() == "nccl" else None)))
        logs = dict(logs, step=self.state.global_step)
        self.log_history.append(logs)
        if getattr(self.args, "local_rank", 0) in (0, -1) and _rank() == 0:
            print({k: (round(v, 6) if isinstance(v, float) else v) for k, v in logs.items()}, flush=True)
        return logs

    # ------------------------------------------------------------------------------------------ step + loop
    def _prepare_inputs(self, inputs):
        dev = self.accelerator.device

        def mv(v):
            if isinstance(v, torch.Tensor):
                return v.to(dev, non_blocking=True)
            if isinstance(v, dict):
                return {k: mv(x) for k, x in v.items()}
            return v
        return {k: mv(v) for k, v in inputs.items()}

    def training_step(self, model, inputs) -> torch.Tensor:
        """reference base/trainer.py:303-308 + transformers Trainer.training_step: H2D, loss, backward, return
        loss.detach() / gradient_accumulation_steps.  (No empty_cache / gc.collect: that flush serialises the device.)"""
        model.train()
        inputs = self._prepare_inputs(inputs)
        loss = self.compute_loss(model, inputs)
        ga = max(1, int(getattr(self.args, "gradient_accumulation_steps", 1) or 1))
        loss.backward()
        return loss.detach() / ga

    def evaluate(self, eval_dataset=None, metric_key_prefix: str = "eval") -> Dict[str, float]:
        """HF Trainer.evaluate: mean eval loss (+ the metrics prediction_step stores: DPO's eight eval_ metrics) over the (rank-sharded) eval set."""
        ds = eval_dataset if eval_dataset is not None else self.eval_dataset
        if not ds:
            return {}
        self._before_evaluate(ds, eval_dataset is not None)
        bs = int(getattr(self.args, "per_device_eval_batch_size", None) or getattr(self.args, "per_device_train_batch_size", 4))
        # the index list is padded by wrapping to a multiple of the world size (as _train_row_batches does): every rank runs the same
        # number of prediction steps and reduces the same 9 scalars in log() - an eval set smaller than the world would otherwise
        # leave ranks without metrics and hang the collective (torch DistributedSampler semantics, as HF's eval dataloader)
        rows = list(ds)
        w = _world()
        if w > 1 and len(rows) % w:
            pad = (-len(rows)) % w                      # cycled: an eval set smaller than the padding still fills every rank
            rows = rows + (rows * (pad // len(rows) + 1))[:pad]
        rows = rows[_rank()::w]
        was_training = self.model.training
        self.model.eval()
        self._evaluate_samples(rows, bs)
        losses = []
        for i in range(0, len(rows), bs):
            loss, _, _ = self.prediction_step(self.model, self.data_collator(rows[i:i + bs]))
            losses.append(loss)
        self.model.train(was_training)
        out = {f"{metric_key_prefix}_loss": float(torch.stack(losses).mean()) if losses else float("nan")}
        return self.log(out)

    def _train_row_batches(self, epoch: int):
        """One epoch of this rank's row batches.  torch DistributedSampler semantics (accelerate MULTI_GPU, ddp.yaml): the
        shuffled index list is padded by wrapping to a multiple of the world size so that EVERY rank gets the same number
        of batches (unequal counts would dead-lock the gradient all-reduce), then strided by rank.  HF's default
        dataloader_drop_last=False: the final partial batch is kept."""
        bs = int(getattr(self.args, "per_device_train_batch_size", 4))
        world, rank = _world(), _rank()
        idx = list(range(len(self.train_dataset)))
        random.Random(int(getattr(self.args, "seed", 42)) + epoch).shuffle(idx)
        if world > 1 and len(idx) % world:
            idx += idx[: world - len(idx) % world]
        idx = idx[rank::world]
        drop_last = bool(getattr(self.args, "dataloader_drop_last", False))
        for i in range(0, len(idx), bs):
            rows = idx[i:i + bs]
            if len(rows) < bs and drop_last:
                break
            yield [self.train_dataset[j] for j in rows]

    def _batches_per_epoch(self) -> int:
        bs = int(getattr(self.args, "per_device_train_batch_size", 4))
        n = -(-len(self.train_dataset) // _world())
        return n // bs if getattr(self.args, "dataloader_drop_last", False) else -(-n // bs)

    def get_train_batches(self, epoch: int, skip: int = 0):
        """collated batches of one epoch.  The collator (image decode + CLIP preprocess) runs `dataloader_prefetch` batches
        ahead on a background thread and the H2D copy goes through a copy stream (base/loader.py); 0 = collate inline."""
        import itertools
        depth = int(getattr(self.args, "dataloader_prefetch", 2) or 0)
        rows_iter = lambda: itertools.islice(self._train_row_batches(epoch), skip, None)   # noqa: E731  (resume: skip consumed batches un-collated)
        if depth <= 0:
            for rows in rows_iter():
                yield self.data_collator(rows)
            return
        from .loader import PrefetchLoader
        yield from PrefetchLoader(rows_iter, self.data_collator, self.accelerator.device, depth)

    def lr_at(self, step: int, total: int) -> float:
        """transformers get_scheduler('cosine' | 'linear' | 'constant') with warmup_ratio / warmup_steps."""
        a = self.args
        base = float(getattr(a, "learning_rate", 5e-5))
        warm = int(getattr(a, "warmup_steps", 0) or 0) or math.ceil(float(getattr(a, "warmup_ratio", 0.0) or 0.0) * total)
        kind = str(getattr(a, "lr_scheduler_type", "linear")).split(".")[-1].lower()
        if step < warm:
            return base * step / max(1, warm)
        prog = (step - warm) / max(1, total - warm)
        if kind == "cosine":
            return base * max(0.0, 0.5 * (1.0 + math.cos(math.pi * prog)))
        if kind.startswith("constant"):
            return base
        return base * max(0.0, 1.0 - prog)

    # ------------------------------------------------------------------------------------------ checkpoints
    def _checkpoint_dirs(self):
        import os
        import re
        out_dir = str(getattr(self.args, "output_dir", "output"))
        if not os.path.isdir(out_dir):
            return []
        found = [(int(m.group(1)), os.path.join(out_dir, d)) for d in os.listdir(out_dir)
                 if (m := re.fullmatch(r"checkpoint-(\d+)", d)) and os.path.isfile(os.path.join(out_dir, d, "trainer_state.json"))]
        return [p for _, p in sorted(found)]

    def save_checkpoint(self, step: int, micro: int, epoch: int, window_len: int = 0):
        """HF Trainer._save_checkpoint for this path: `output_dir/checkpoint-<step>/` with the weights (adapters under LoRA),
        the optimizer state (fp32 master / m / v + step), trainer_state.json (step counters, log history, the dropout call counters
        that seed the counter-based masks and the call counter of the NEFTune noise, world size / accumulation steps the counters were taken under); rotated to
        `save_total_limit`.  Rank 0 writes (every rank holds identical state under DDP)."""
        import json
        import os
        import shutil
        from safetensors.torch import save_file
        if _rank() != 0:
            return None
        eng = self.model.engine
        path = os.path.join(str(getattr(self.args, "output_dir", "output")), f"checkpoint-{step}")
        tmp = path + ".tmp"
        shutil.rmtree(tmp, ignore_errors=True)
        os.makedirs(tmp)
        if self.is_peft_model:
            self.model.save_adapter(tmp)
        else:
            self.model.save_pretrained(tmp)
        st = eng.optimizer_state()
        if st is not None:
            for k in ("master", "m", "v"):          # one file per buffer: 27 GB each at 7B full fine-tuning
                save_file({k: st[k].detach().cpu()}, os.path.join(tmp, f"optimizer_{k}.safetensors"))
        with open(os.path.join(tmp, "trainer_state.json"), "w") as f:
            json.dump(dict(global_step=step, micro_step=micro, epoch=epoch, opt_step=eng.opt_step, log_history=self.log_history,
                           world_size=_world(), lora_calls=getattr(eng, "_lora_calls", 0), plora_calls=getattr(eng, "_plora_calls", 0),
                           neftune_calls=getattr(eng, "_neftune_calls", 0),
                           gradient_accumulation_steps=max(1, int(getattr(self.args, "gradient_accumulation_steps", 1) or 1)),
                           per_device_train_batch_size=int(getattr(self.args, "per_device_train_batch_size", 4))), f, indent=1)
        shutil.rmtree(path, ignore_errors=True)
        os.replace(tmp, path)                        # a checkpoint directory is either complete or absent
        limit = int(getattr(self.args, "save_total_limit", 0) or 0)
        if limit > 0:
            for old in self._checkpoint_dirs()[:-limit]:
                shutil.rmtree(old, ignore_errors=True)
        return path

    def load_checkpoint(self, path: str) -> dict:
        import json
        import os
        from safetensors.torch import load_file
        eng = self.model.engine
        with open(os.path.join(path, "trainer_state.json")) as f:
            state = json.load(f)
        # micro_step -> (epoch, batches to skip) only means the same thing under the same sharding
        for key, now in (("world_size", _world()), ("gradient_accumulation_steps", max(1, int(getattr(self.args, "gradient_accumulation_steps", 1) or 1))),
                         ("per_device_train_batch_size", int(getattr(self.args, "per_device_train_batch_size", 4)))):
            if key in state and int(state[key]) != now:
                raise ValueError(f"resume_from_checkpoint: {path} was written with {key}={state[key]}, this run has {now}")
        if self.is_peft_model:
            self.model.load_adapter(path)
        else:
            sd = {}
            for fn in sorted(os.listdir(path)):
                if fn.startswith("model") and fn.endswith(".safetensors"):
                    sd.update(load_file(os.path.join(path, fn)))
            eng.policy.load_state_dict(sd)
        if os.path.isfile(os.path.join(path, "optimizer_master.safetensors")):
            bufs = {k: load_file(os.path.join(path, f"optimizer_{k}.safetensors"))[k] for k in ("master", "m", "v")}
            eng.load_optimizer_state(bufs["master"], bufs["m"], bufs["v"], state["opt_step"])
        if hasattr(eng, "_lora_calls"):
            eng._lora_calls = int(state.get("lora_calls", 0))
        if hasattr(eng, "_plora_calls"):
            eng._plora_calls = int(state.get("plora_calls", 0))
        if hasattr(eng, "_neftune_calls"):
            eng._neftune_calls = int(state.get("neftune_calls", 0))
        self.log_history = list(state.get("log_history", []))
        return state

    def train(self, resume_from_checkpoint=None):
        """the step loop; NEFTune (neftune_noise_alpha) is on from _before_train to the return, as in transformers Trainer.train"""
        try:
            return self._train(resume_from_checkpoint)
        finally:
            self._deactivate_neftune()

    def _train(self, resume_from_checkpoint=None):
        a = self.args
        eng = self.model.engine
        ga = max(1, int(getattr(a, "gradient_accumulation_steps", 1) or 1))
        n_batches = self._batches_per_epoch()
        if n_batches == 0:
            raise ValueError(f"the training set ({len(self.train_dataset)} rows over {_world()} rank(s)) yields no batch of "
                             f"per_device_train_batch_size={getattr(a, 'per_device_train_batch_size', 4)} with dataloader_drop_last")
        per_epoch = max(1, n_batches // ga)
        max_steps = int(getattr(a, "max_steps", -1) or -1)
        epochs = float(getattr(a, "num_train_epochs", 1.0))
        total = max_steps if max_steps > 0 else int(math.ceil(per_epoch * epochs))
        logging_steps = max(1, int(getattr(a, "logging_steps", 10) or 10))
        save_strategy = str(getattr(a, "save_strategy", "no")).split(".")[-1].lower()
        save_steps = max(1, int(getattr(a, "save_steps", 500) or 500))
        self._before_train()
        eng.init_optimizer() if eng.master is None else None
        eng.zero_grad()
        step, micro, ep = 0, 0, 0
        skip = 0              # micro-batches of the resumed epoch that were already consumed
        if resume_from_checkpoint:
            ckpt = resume_from_checkpoint if isinstance(resume_from_checkpoint, str) else (self._checkpoint_dirs() or [None])[-1]
            if ckpt is None:
                raise ValueError(f"resume_from_checkpoint: no checkpoint-* directory under {getattr(a, 'output_dir', 'output')}")
            st = self.load_checkpoint(ckpt)
            step, micro = int(st["global_step"]), int(st["micro_step"])
            ep, skip = divmod(micro, n_batches)
            self.state.global_step = step
        last_saved = [-1]

        def save(step_, micro_, ep_):
            last_saved[0] = step_
            return self.save_checkpoint(step_, micro_, ep_)

        window = []           # device scalars; only read back at logging time (no per-step host sync)
        epoch_save_due = False
        while step < total:
            it = iter(self.get_train_batches(ep, skip=skip))
            nxt = next(it, None)
            while nxt is not None:
                batch = nxt
                if eng.reducer is not None:        # DDP no_sync: reduce only with the last micro-batch of an accumulation window
                    eng.reducer.enabled = (micro + 1) % ga == 0
                window.append(self.training_step(self.model, batch))
                nxt = next(it, None)
                if nxt is not None:                # look-ahead of one batch: its reference forward runs under the optimizer step
                    nxt = self.prefetch_reference(nxt)
                micro += 1
                if micro % ga:
                    continue
                lr = self.lr_at(step, total)
                eng.optimizer_step(lr=lr, beta1=float(getattr(a, "adam_beta1", 0.9)), beta2=float(getattr(a, "adam_beta2", 0.999)),
                                   eps=float(getattr(a, "adam_epsilon", 1e-8)), weight_decay=float(getattr(a, "weight_decay", 0.0)),
                                   max_grad_norm=float(getattr(a, "max_grad_norm", 1.0) or 0.0),
                                   grad_scale=(1.0 / (ga * _world())) if eng.reducer is not None else 1.0 / ga)
                step += 1
                self.state.global_step = step
                if step % logging_steps == 0 or step >= total:
                    n_opt = max(1, len(window) // ga)
                    self.log({"loss": float(torch.stack(window).sum()) / n_opt, "learning_rate": lr,
                              "grad_norm": eng.grad_norm(), "epoch": micro / ga / per_epoch})
                    window = []
                ev = str(getattr(a, "evaluation_strategy", "no")).split(".")[-1].lower()
                if ev == "steps" and self.eval_dataset and step % max(1, int(getattr(a, "eval_steps", None) or logging_steps)) == 0:
                    self.evaluate()
                if save_strategy == "steps" and step % save_steps == 0:
                    save(step, micro, ep)
                elif epoch_save_due:                    # the epoch ended inside an accumulation window: saved at the first optimizer step after it
                    save(step, micro, ep)
                epoch_save_due = False
                if step >= total:
                    break
            # HF fires on_epoch_end - and with save_strategy="epoch" saves - at every epoch end INCLUDING the one training stops in, whether
            # the epoch was consumed or max_steps cut it short (the loop leaves on an optimizer-step boundary in both cases).  A checkpoint is
            # only state at such a boundary: an epoch that ends inside an accumulation window defers its save to the next optimizer step.
            if save_strategy == "epoch":
                if step >= total:
                    if last_saved[0] != step:
                        save(step, micro, ep)
                elif micro % ga == 0:
                    save(step, micro, ep)
                else:
                    epoch_save_due = True
                    if _rank() == 0:
                        print(f"[vlrlhf] epoch {ep} ended inside an accumulation window ({micro % ga} of {ga} micro-batches): its checkpoint is written at optimizer step {step + 1}", flush=True)
            ep += 1
            skip = 0
        return self.state

    def save_state(self):
        """HF Trainer.save_state: trainer_state.json (step counter + log history) in output_dir, rank 0."""
        import json
        import os
        if _rank() != 0:
            return
        out_dir = str(getattr(self.args, "output_dir", "output"))
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "trainer_state.json"), "w") as f:
            json.dump(dict(global_step=self.state.global_step, log_history=self.log_history), f, indent=1)

    def add_callback(self, cb):
        self.callbacks.append(cb)


class VLDPOTrainer(VLTrainerLoop):
    def __init__(
        self,
        model=None,
        ref_model=None,
        beta: float = 0.1,
        label_smoothing: float = 0,
        loss_type: Literal["sigmoid", "hinge", "ipo", "kto_pair", "ddpo"] = "sigmoid",
        args=None,
        data_collator: Any = None,
        label_pad_token_id: int = -100,
        padding_value: int = None,
        truncation_mode: str = "keep_end",
        train_dataset=None,
        eval_dataset=None,
        processor=None,
        model_init: Optional[Callable] = None,
        callbacks: Optional[List] = None,
        optimizers: Tuple = (None, None),
        preprocess_logits_for_metrics: Optional[Callable] = None,
        max_length: Optional[int] = None,
        max_prompt_length: Optional[int] = None,
        max_target_length: Optional[int] = None,
        peft_config: Optional[Dict] = None,
        is_encoder_decoder: Optional[bool] = None,
        disable_dropout: bool = True,
        generate_during_eval: bool = False,
        compute_metrics: Optional[Callable] = None,
        precompute_ref_log_probs: bool = False,
        dataset_num_proc: Optional[int] = None,
        model_init_kwargs: Optional[Dict] = None,
        ref_model_init_kwargs: Optional[Dict] = None,
        model_adapter_name: Optional[str] = None,
        ref_adapter_name: Optional[str] = None,
        reference_free: bool = False,
    ):
        # argument order = reference base/trainer.py:34-68 (MyAutoDPOTrainer passes them positionally)
        if model is None:
            raise ValueError("VLDPOTrainer needs a model")
        if peft_config is not None:
            # trl==0.8.1 DPOTrainer.__init__: model = get_peft_model(model, peft_config); with a peft policy and no
            # ref_model the reference pass runs the policy with its adapters disabled (null_ref_context)
            if not hasattr(model, "apply_lora"):
                raise ValueError("peft_config given but the model wrapper has no apply_lora()")
            model.apply_lora(peft_config)
        self.is_peft_model = bool(getattr(model, "is_peft_model", False))
        self._init_neftune(model, args)          # transformers Trainer: args.neftune_noise_alpha (the policy's training passes only)
        self.processor = processor
        self.tokenizer = processor.tokenizer if processor is not None else None
        self.model = model
        self.beta = beta
        self.label_smoothing = label_smoothing
        self.loss_type = loss_type
        self.args = args
        self.label_pad_token_id = label_pad_token_id
        self.padding_value = padding_value if padding_value is not None else (
            self.tokenizer.pad_token_id if self.tokenizer is not None and self.tokenizer.pad_token_id is not None else 0)
        self.truncation_mode = truncation_mode
        self.max_length = max_length if max_length is not None else 512
        self.max_prompt_length = max_prompt_length if max_prompt_length is not None else 128
        self.max_target_length = max_target_length
        self.is_encoder_decoder = bool(is_encoder_decoder) if is_encoder_decoder is not None else bool(
            getattr(getattr(model, "config", None), "is_encoder_decoder", False))
        if self.is_encoder_decoder:
            raise NotImplementedError("encoder-decoder models are not on the MI355X DPO path")
        self.generate_during_eval = generate_during_eval
        self.precompute_ref_log_probs = precompute_ref_log_probs
        self._precomputed_train_ref_log_probs = False
        self._precomputed_eval_ref_log_probs = False
        self.reference_free = reference_free
        self.dataset_num_proc = dataset_num_proc
        self.callbacks = list(callbacks or [])
        self.use_dpo_data_collator = True
        self._stored_metrics = defaultdict(lambda: defaultdict(list))
        self.log_history: List[dict] = []
        self.accelerator = _Accelerator(model)
        # trl: ref_model None and no peft -> frozen deep copy of the policy
        if ref_model is None and not reference_free and not precompute_ref_log_probs and not self.is_peft_model:
            ref_model = model.create_reference_model() if hasattr(model, "create_reference_model") else None
        self.ref_model = ref_model
        self.data_collator = data_collator
        self.train_dataset = self._tokenize_dataset(train_dataset)
        self.eval_dataset = self._tokenize_dataset(eval_dataset)
        self.ref_on_side_stream = True
        self._ref_stream = None
        # VLR_REF_PIPELINE=1: reference forward of the NEXT batch issued between the backward and the optimizer step of the
        # current one (prefetch_reference), so the HBM-bound clip + AdamW pass runs under the frozen forward.  Bit-identical
        # results, but OFF by default: measured +6 ms per step at N=1 (638.0 vs 632.1 ms, same box) - the
        # persistent GEMM workgroups fill the register file of every CU, so AdamW blocks do not co-reside with them, they
        # displace them, and the persistent tile walk pays a tail for every displaced workgroup.
        self.ref_pipeline = os.environ.get("VLR_REF_PIPELINE", "0") == "1"
        self._ref_pending = None
        self.state = _State()

    # ------------------------------------------------------------------------------------------ tokenisation
    def _tokenize_dataset(self, ds):
        if ds is None:
            return None
        rows = list(ds)
        if rows and "chosen_input_ids" not in rows[0]:
            rows = [self.tokenize_row(dict(r)) for r in rows]
        return rows

    def build_tokenized_answer(self, prompt: str, answer: str) -> Dict:
        """trl==0.8.1 DPOTrainer.build_tokenized_answer: tokenize prompt+answer jointly and split so that
        enc(prompt) + enc(answer) == enc(prompt + answer) even when the tokenizer merges across the boundary."""
        full = self.tokenizer(prompt + answer, add_special_tokens=False)
        prompt_ids = self.tokenizer(prompt, add_special_tokens=False)["input_ids"]
        answer_ids = full["input_ids"][len(prompt_ids):]
        answer_mask = full["attention_mask"][len(prompt_ids):]
        if len(full["input_ids"]) != len(prompt_ids + answer_ids):
            raise ValueError("Prompt input ids and answer input ids should have the same length.")
        start = len(prompt_ids)
        if prompt_ids != full["input_ids"][:start]:
            start -= 1
        p_ids, p_mask = full["input_ids"][:start], full["attention_mask"][:start]
        if len(p_ids) != len(p_mask):
            raise ValueError("Prompt input ids and attention mask should have the same length.")
        return dict(prompt_input_ids=p_ids, prompt_attention_mask=p_mask,
                    input_ids=full["input_ids"][start:], attention_mask=full["attention_mask"][start:] if answer_mask is not None else None)

    def _trl_tokenize_row(self, feature) -> Dict:
        """trl==0.8.1 DPOTrainer.tokenize_row, decoder-only branch (the reference restates the same truncation / label
        logic in-repo at models/QwenVL/__init__.py:281-347)."""
        prompt, chosen, rejected = feature["prompt"], feature["chosen"], feature["rejected"]
        if not isinstance(prompt, str):
            raise ValueError(f"prompt should be an str but got {type(prompt)}")
        tok = self.tokenizer
        prompt_tokens = {f"prompt_{k}": v for k, v in tok(prompt, add_special_tokens=False).items()}
        if not isinstance(chosen, str):
            raise ValueError(f"chosen should be an str but got {type(chosen)}")
        chosen_tokens = self.build_tokenized_answer(prompt, chosen)
        if not isinstance(rejected, str):
            raise ValueError(f"rejected should be an str but got {type(rejected)}")
        rejected_tokens = self.build_tokenized_answer(prompt, rejected)
        c_len, r_len = len(chosen_tokens["prompt_input_ids"]), len(rejected_tokens["prompt_input_ids"])
        p_len = min(c_len, r_len)
        for k in ("prompt_input_ids", "prompt_attention_mask"):
            prompt_tokens[k] = prompt_tokens[k][:p_len]
        ndiff = sum(a != b for a, b in zip(chosen_tokens["prompt_input_ids"], rejected_tokens["prompt_input_ids"]))
        if ndiff > 1 or abs(c_len - r_len) > 1:
            raise ValueError("Chosen and rejected prompt_input_ids might only differ on the last token due to tokenizer "
                             "merge ops.")
        bos, eos = tok.bos_token_id, tok.eos_token_id
        for t in (prompt_tokens, chosen_tokens, rejected_tokens):
            t["prompt_input_ids"] = [bos] + list(t["prompt_input_ids"])
            t["prompt_attention_mask"] = [1] + list(t["prompt_attention_mask"])
        for t in (chosen_tokens, rejected_tokens):
            t["input_ids"] = list(t["input_ids"]) + [eos]
            t["attention_mask"] = list(t["attention_mask"]) + [1]
        longer = max(len(chosen_tokens["input_ids"]), len(rejected_tokens["input_ids"]))
        for t in (chosen_tokens, rejected_tokens, prompt_tokens):
            if len(t["prompt_input_ids"]) + longer > self.max_length:
                if self.truncation_mode == "keep_start":
                    for k in ("prompt_input_ids", "prompt_attention_mask"):
                        t[k] = t[k][: self.max_prompt_length]
                elif self.truncation_mode == "keep_end":
                    for k in ("prompt_input_ids", "prompt_attention_mask"):
                        t[k] = t[k][-self.max_prompt_length:]
                else:
                    raise ValueError(f"Unknown truncation mode: {self.truncation_mode}")
        for t in (chosen_tokens, rejected_tokens):
            if len(t["prompt_input_ids"]) + longer > self.max_length:
                for k in ("input_ids", "attention_mask"):
                    t[k] = t[k][: self.max_length - self.max_prompt_length]
        batch = {}
        for name, t in (("chosen_", chosen_tokens), ("rejected_", rejected_tokens)):
            seq_ids = t["prompt_input_ids"] + t["input_ids"]
            seq_mask = t["prompt_attention_mask"] + t["attention_mask"]
            labels = list(seq_ids)
            n = len(t["prompt_input_ids"])
            labels[:n] = [self.label_pad_token_id] * n
            batch[name + "input_ids"], batch[name + "attention_mask"], batch[name + "labels"] = seq_ids, seq_mask, labels
        batch["prompt_input_ids"] = prompt_tokens["prompt_input_ids"]
        batch["prompt_attention_mask"] = prompt_tokens["prompt_attention_mask"]
        return batch

    def tokenize_row(self, feature, model=None) -> Dict:
        """reference base/trainer.py:105-122."""
        prompt = self.processor.format_multimodal_prompt(feature["prompt"], feature["img_path"])
        conv = self.processor.make_single_turn_conv(prompt, "")
        raw = self.processor.process_batch_conv([conv], system_message=None, add_end_for_empty_value=False)["raw_str"][0]
        end = self.processor.chat_template.assistant_end
        feature = dict(feature)
        feature["chosen"] += end
        feature["rejected"] += end
        feature["prompt"] = raw
        batch = self._trl_tokenize_row(feature)
        batch["img_path"] = feature["img_path"]
        for k in ("reference_chosen_logps", "reference_rejected_logps"):
            if k in feature:
                batch[k] = feature[k]
        return batch

    # ------------------------------------------------------------------------------------------ batching
    def concatenated_inputs(self, batch, is_encoder_decoder: bool = False, label_pad_token_id: int = -100,
                            padding_value: int = 0, device=None) -> Dict[str, torch.Tensor]:
        """reference base/trainer.py:124-146 (+ trl static base): chosen over rejected, padded to the common length;
        every image tensor / list is duplicated on the batch dimension.  The duplicate carries `_vlr_dup = 2` so the
        frozen vision tower is evaluated once per distinct image (results identical), and the result is memoised on
        the batch so the policy pass and the reference pass share the same device tensors."""
        cache = batch.get("_vlr_concat") if isinstance(batch, dict) else None
        src_ids = tuple(id(batch.get(k)) for k in ("chosen_input_ids", "rejected_input_ids", "chosen_labels", "rejected_labels",
                                                    "chosen_attention_mask", "rejected_attention_mask", "img_input_dict"))
        if cache is not None and cache.get("_vlr_src") == src_ids:     # a dict(batch) copy with replaced tensors must not hit
            return {k: v for k, v in cache.items() if k != "_vlr_src"}
        out = {}
        n = max(batch["chosen_input_ids"].shape[1], batch["rejected_input_ids"].shape[1])
        for field, pad in (("input_ids", padding_value), ("attention_mask", 0), ("labels", label_pad_token_id)):
            parts = [pad_to_length(batch[f"{s}_{field}"], n, pad) for s in ("chosen", "rejected")]
            t = torch.cat(parts, dim=0)
            out[f"concatenated_{field}"] = t.to(device) if device is not None else t
        # integer facts about THIS batch that every pass over it needs on the host (merged length, lm-head row count, DDPO
        # mask ...): the first pass computes them (one D2H each), later passes - the policy pass after the reference pass, the
        # next visit of a resident batch - read them here instead of stalling the device again
        out["concatenated_input_ids"]._vlr_meta = {}
        if "img_input_dict" in batch:
            d = {}
            for k, v in batch["img_input_dict"].items():
                if isinstance(v, torch.Tensor):
                    t = torch.cat([v, v], dim=0)
                    t = t.to(device) if device is not None else t
                    t._vlr_dup = 2
                    d[k] = t
                elif isinstance(v, list):
                    d[k] = v + v
                else:
                    raise ValueError(f"Unsupported type {type(v)} for concatenation.")
            out["concatenated_img_input_dict"] = d
        if isinstance(batch, dict):
            batch["_vlr_concat"] = dict(out, _vlr_src=src_ids)
        return out

    @staticmethod
    def get_batch_logps(logits, labels, average_log_prob: bool = False, label_pad_token_id: int = -100,
                        is_encoder_decoder: bool = False, mask_shared_tokens: bool = False) -> torch.Tensor:
        """reference base/trainer.py:148-188.  `logits` is either the lazy lm-head handle the MI355X model wrappers
        return (fused path: the [2B,S,V] tensor is never materialised) or a real [2B,S,V] tensor on the GPU."""
        if tuple(logits.shape[:-1]) != tuple(labels.shape):
            raise ValueError("Logits (batch and sequence length dim) and labels must have the same shape.")
        if is_encoder_decoder:
            raise NotImplementedError("encoder-decoder models are not on the MI355X DPO path")
        shared = None
        if mask_shared_tokens:
            assert labels.shape[0] % 2 == 0
            meta = getattr(labels, "_vlr_meta", None)
            shared = meta.get("ddpo_mask") if meta is not None else None
            if shared is None:
                shared = ddpo_shared_mask(labels, label_pad_token_id, min_match_size=3)
                if meta is not None:
                    meta["ddpo_mask"] = shared.to(labels.device) if labels.is_cuda else shared
        if hasattr(logits, "batch_logps"):
            return logits.batch_logps(labels, shared, average_log_prob, label_pad_token_id)
        if not logits.is_cuda:
            raise _hip.VlrError("get_batch_logps: logits must live on the MI355X (no CPU fallback)")
        return _TensorLogpsFn.apply(logits, labels, shared, bool(average_log_prob), int(label_pad_token_id))

    def concatenated_forward(self, model, batch):
        """reference base/trainer.py:190-242."""
        cb = self.concatenated_inputs(batch, is_encoder_decoder=self.is_encoder_decoder,
                                      label_pad_token_id=self.label_pad_token_id, padding_value=self.padding_value,
                                      device=self.accelerator.device)
        len_chosen = batch["chosen_labels"].shape[0]
        kwargs = {"use_cache": False}
        if "concatenated_img_input_dict" in cb:
            kwargs.update(cb["concatenated_img_input_dict"])
        output = model(input_ids=cb["concatenated_input_ids"], attention_mask=cb["concatenated_attention_mask"],
                       labels=cb["concatenated_labels"], **kwargs)
        all_logits = output.logits
        final_labels = output.labels if getattr(output, "labels", None) is not None else cb["concatenated_labels"]
        all_logps = self.get_batch_logps(all_logits, final_labels, average_log_prob=False,
                                         is_encoder_decoder=self.is_encoder_decoder,
                                         label_pad_token_id=self.label_pad_token_id,
                                         mask_shared_tokens=self.loss_type == "ddpo")
        return (all_logps[:len_chosen], all_logps[len_chosen:], all_logits[:len_chosen], all_logits[len_chosen:])

    def dpo_loss(self, policy_chosen_logps, policy_rejected_logps, reference_chosen_logps, reference_rejected_logps):
        """reference base/trainer.py:244-301 -> (losses, chosen_rewards, rejected_rewards)."""
        if self.loss_type not in LOSS_TYPE_IDS:
            raise ValueError(
                f"Unknown loss type: {self.loss_type}. Should be one of ['sigmoid', 'hinge', 'ipo', 'kto_pair']")
        dev = self.accelerator.device
        return _DpoLossFn.apply(policy_chosen_logps.to(dev), policy_rejected_logps.to(dev),
                                reference_chosen_logps.to(dev), reference_rejected_logps.to(dev), self.beta,
                                self.label_smoothing, LOSS_TYPE_IDS[self.loss_type], self.reference_free)

    # ------------------------------------------------------------------------------------------ loss + metrics
    def _reference_logps(self, batch):
        if "reference_chosen_logps" in batch and "reference_rejected_logps" in batch:
            dev = self.accelerator.device
            return batch["reference_chosen_logps"].to(dev).float(), batch["reference_rejected_logps"].to(dev).float()
        if self.ref_model is None:
            if not self.is_peft_model:
                raise ValueError("no reference model and no precomputed reference log-probs in the batch")
            with torch.no_grad(), self.null_ref_context(), self._reference_pass(self.model):
                rc, rr, _, _ = self.concatenated_forward(self.model, batch)
            return rc, rr
        with torch.no_grad(), self._reference_pass(self.ref_model):
            rc, rr, _, _ = self.concatenated_forward(self.ref_model, batch)
        return rc, rr

    @staticmethod
    def _reference_pass(owner):
        """a reference forward reads nothing but its log-probs: models that can skip the duplicate prompt rows of each pair
        (LlavaForRL.reference_pass) are told so for the duration of the call"""
        return owner.reference_pass() if hasattr(owner, "reference_pass") else contextlib.nullcontext()

    @staticmethod
    def _policy_pass(owner):
        """the policy forward of a DPO step is back-propagated as a whole and reads the two sequences of every pair: models that can run
        the pair's shared prompt rows once, forward and backward (LlavaForRL.policy_pass), are told so for the duration of the call"""
        return owner.policy_pass() if hasattr(owner, "policy_pass") else contextlib.nullcontext()

    def null_ref_context(self):
        """trl==0.8.1 DPOTrainer.null_ref_context: the peft policy with its adapters disabled is the reference model."""
        return self.model.disable_adapter() if self.is_peft_model else contextlib.nullcontext()

    def _ref_owner(self):
        return self.ref_model if self.ref_model is not None else (self.model if self.is_peft_model else None)

    def _ref_side_ok(self, batch) -> bool:
        return bool(self.ref_on_side_stream and self._ref_owner() is not None and "reference_chosen_logps" not in batch
                    and torch.cuda.is_available())

    def _launch_reference(self, batch):
        """the frozen reference forward on the side HIP stream, ordered after everything queued on the current stream so far
        (the shared ViT features are evaluated there first)"""
        main = torch.cuda.current_stream()
        ref_owner = self._ref_owner()
        cb = self.concatenated_inputs(batch, False, self.label_pad_token_id, self.padding_value, self.accelerator.device)
        if "concatenated_img_input_dict" in cb and hasattr(ref_owner, "prefetch_vision"):
            ref_owner.prefetch_vision(cb["concatenated_img_input_dict"])
        if self._ref_stream is None:
            self._ref_stream = torch.cuda.Stream()
        self._ref_stream.wait_stream(main)
        with torch.cuda.stream(self._ref_stream):
            return self._reference_logps(batch)

    def prefetch_reference(self, inputs):
        """Issue the reference forward of the NEXT batch now.  Called by the training loop (and bench.py) after the backward of
        the current batch is queued and BEFORE the optimizer step: the reference model is frozen (under LoRA: the base weights
        with the adapters disabled), so its log-probs do not depend on the update, and the HBM-bound gradient-norm + AdamW pass
        (and, N > 1, the exposed tail of the gradient all-reduce) overlaps the compute-bound forward instead of idling the MFMA
        units.  Returns the device-resident batch to hand to training_step(); a batch that is never trained on just drops its
        result.  Work per optimizer step is unchanged: one reference forward, one policy forward + backward, one update."""
        inputs = self._prepare_inputs(inputs)
        if self.ref_pipeline and self._ref_side_ok(inputs) and "chosen_input_ids" in inputs:
            rc, rr = self._launch_reference(inputs)
            self._ref_pending = (inputs["chosen_input_ids"], rc, rr)
        return inputs

    def _before_train(self):
        if self.precompute_ref_log_probs and not self._precomputed_train_ref_log_probs:
            self.precompute_reference_log_probs(self.train_dataset)
            self._precomputed_train_ref_log_probs = True
        super()._before_train()

    def _before_evaluate(self, ds, explicit: bool):
        if self.precompute_ref_log_probs and not self._precomputed_eval_ref_log_probs and not explicit:
            self.precompute_reference_log_probs(ds)
            self._precomputed_eval_ref_log_probs = True

    def _evaluate_samples(self, rows, bs):
        if self.generate_during_eval and rows:
            # trl==0.8.1 DPOTrainer.evaluation_loop: ONE random eval batch is sampled from the policy and the reference and logged as a
            # (prompt, policy, reference) table (wandb.Table there; a "game_log" entry of log_history + a rank-0 print here).  Every rank
            # draws its own batch from its shard - no collective is involved.
            import random
            pick = random.sample(range(len(rows)), k=min(bs, len(rows)))
            sample = self._prepare_inputs(self.data_collator([rows[i] for i in pick]))
            policy_txt, ref_txt = self.get_batch_samples(self.model, sample)
            prompts = sample.get("prompt") or self.tokenizer.batch_decode(sample["prompt_input_ids"], skip_special_tokens=True)
            table = [[pr, po[len(pr):], rf[len(pr):]] for pr, po, rf in zip(prompts, policy_txt, ref_txt)]
            if _rank() == 0:
                self.log_history.append({"game_log": {"columns": ["Prompt", "Policy", "Ref Model"], "rows": table}, "step": self.state.global_step})
                for row in table:
                    print({"prompt": row[0], "policy": row[1], "ref_model": row[2]}, flush=True)

    def get_batch_loss_metrics(self, model, batch, train_eval: Literal["train", "eval"] = "train"):
        """trl==0.8.1 DPOTrainer.get_batch_loss_metrics.  The reference forward is issued on a side HIP stream ahead of
        the policy forward (it is frozen and shares only the cached vision features), then joined before the loss."""
        main = torch.cuda.current_stream()
        pending, use_side = self._ref_pending, False
        if pending is not None and pending[0] is batch.get("chosen_input_ids"):
            rc, rr = pending[1], pending[2]             # issued by prefetch_reference during the previous step
            self._ref_pending = None
            use_side = True
        elif self._ref_side_ok(batch):
            rc, rr = self._launch_reference(batch)
            use_side = True
        with self._policy_pass(model):
            pc, pr, pcl, prl = self.concatenated_forward(model, batch)
        if use_side:
            main.wait_stream(self._ref_stream)
            rc.record_stream(main)
            rr.record_stream(main)
        else:
            rc, rr = self._reference_logps(batch)
        losses, chosen_rewards, rejected_rewards = self.dpo_loss(pc, pr, rc, rr)
        reward_accuracies = (chosen_rewards > rejected_rewards).float()
        prefix = "eval_" if train_eval == "eval" else ""
        metrics = {
            f"{prefix}rewards/chosen": chosen_rewards.mean(),
            f"{prefix}rewards/rejected": rejected_rewards.mean(),
            f"{prefix}rewards/accuracies": reward_accuracies.mean(),
            f"{prefix}rewards/margins": (chosen_rewards - rejected_rewards).mean(),
            f"{prefix}logps/rejected": pr.detach().mean(),
            f"{prefix}logps/chosen": pc.detach().mean(),
            f"{prefix}logits/rejected": prl.detach().mean(),
            f"{prefix}logits/chosen": pcl.detach().mean(),
        }
        return losses.mean(), metrics

    def compute_loss(self, model, inputs, return_outputs: bool = False):
        loss, metrics = self.get_batch_loss_metrics(model, inputs, train_eval="train")
        self.store_metrics(metrics, train_eval="train")
        if return_outputs:
            return loss, metrics
        return loss

    # ------------------------------------------------------------------------------------------ evaluation
    def prediction_step(self, model, inputs, prediction_loss_only: bool = True, ignore_keys=None):
        """trl==0.8.1 DPOTrainer.prediction_step: no-grad loss + metrics of one batch, stored under the eval_ prefix;
        returns (loss, logits, labels) with logits = [eval_logits/chosen, eval_logits/rejected] as trl does."""
        with torch.no_grad():
            loss, metrics = self.get_batch_loss_metrics(model, self._prepare_inputs(inputs), train_eval="eval")
        self.store_metrics(metrics, train_eval="eval")
        if prediction_loss_only:
            return loss.detach(), None, None
        logits = torch.stack([metrics["eval_logits/chosen"], metrics["eval_logits/rejected"]]).mean(dim=0, keepdim=True)
        return loss.detach(), logits, torch.zeros(logits.shape[0], device=logits.device)

    # ------------------------------------------------------------------------------------------ reference pre-pass
    def compute_reference_log_probs(self, padded_batch: Dict) -> Tuple[torch.Tensor, torch.Tensor]:
        """trl==0.8.1 DPOTrainer.compute_reference_log_probs: reference log-probs of one collated batch, no grad.  Without
        a ref_model the policy itself is the reference (its adapters disabled if it is a peft model): the pre-pass runs
        before the first optimizer step, so these are the initial weights."""
        with torch.no_grad():
            if self.ref_model is None:
                with self.null_ref_context(), self._reference_pass(self.model):
                    was_training = self.model.training
                    self.model.eval()
                    rc, rr, _, _ = self.concatenated_forward(self.model, padded_batch)
                    self.model.train(was_training)
            else:
                with self._reference_pass(self.ref_model):
                    rc, rr, _, _ = self.concatenated_forward(self.ref_model, padded_batch)
        return rc, rr

    def precompute_reference_log_probs(self, dataset, batch_size: Optional[int] = None):
        """trl==0.8.1 get_train_dataloader / get_eval_dataloader with precompute_ref_log_probs=True: one no-grad pass over
        the tokenised dataset, the two log-probs are stored on every row as `reference_chosen_logps` /
        `reference_rejected_logps`; the collator turns them into float tensors and the training step then skips the
        reference forward (21 % of the step at the 7B configuration).  Every rank walks the whole dataset, as in trl."""
        if dataset is None or not len(dataset) or "reference_chosen_logps" in dataset[0]:
            return dataset
        bs = int(batch_size or getattr(self.args, "per_device_eval_batch_size", None) or
                 getattr(self.args, "per_device_train_batch_size", 4))
        for i in range(0, len(dataset), bs):
            rows = dataset[i:i + bs]
            batch = self._prepare_inputs(self.data_collator(rows))
            rc, rr = self.compute_reference_log_probs(batch)
            rc, rr = rc.float().cpu().tolist(), rr.float().cpu().tolist()
            for r, c, j in zip(rows, rc, rr):
                r["reference_chosen_logps"], r["reference_rejected_logps"] = c, j
        return dataset

    def get_batch_samples(self, model, batch):
        """reference base/trainer.py:310-360: sample a continuation of every prompt from the policy and from the reference (the batch's
        `reference_output`, else the reference model, else the policy with its adapters disabled), pad to max_length, decode.
        Evaluation-time only (`generate_during_eval`; the reference CLI never switches it on): `model.generate` decodes with its KV cache
        where the model has one (LLaVA-1.5 / LLaVA-Next: one prefill, then one decode step per token) and re-runs the HIP forward per
        token otherwise."""
        others = dict(batch.get("img_input_dict", {}))
        kw = dict(input_ids=batch["prompt_input_ids"], attention_mask=batch["prompt_attention_mask"], max_length=self.max_length,
                  do_sample=True, pad_token_id=self.tokenizer.pad_token_id, **others)
        # the stop token is the TOKENIZER's (Qwen-VL's HF config has no eos_token_id: its end token is tokenizer.eod_id; the model-side
        # default of `generate` is LLaMA's id 2)
        eos = getattr(self.tokenizer, "eos_token_id", None)
        if eos is None:
            eos = getattr(self.tokenizer, "eod_id", None)
        if eos is not None:
            kw["eos_token_id"] = eos
        # merge_lora=False: sampling inside training must not clone the policy - the adapters run live in the prefill and in every decode step
        policy_output = model.generate(merge_lora=False, **kw)
        if "reference_output" in batch:
            reference_output = batch["reference_output"]
        elif self.ref_model is None:
            with self.null_ref_context():
                reference_output = self.model.generate(**kw)
        else:
            reference_output = self.ref_model.generate(**kw)
        pad = self.tokenizer.pad_token_id
        policy_output = pad_to_length(policy_output, self.max_length, pad)
        reference_output = pad_to_length(reference_output, self.max_length, pad)
        return (self.tokenizer.batch_decode(policy_output, skip_special_tokens=True),
                self.tokenizer.batch_decode(reference_output, skip_special_tokens=True))


class VLSFTTrainer(VLTrainerLoop):
    """Supervised fine-tuning - mirror of the reference src/vlrlhf/base/trainer.py:573-674 plus what the reference inherits from
    trl==0.8.1 `SFTTrainer` / transformers `Trainer` on this path: loss = the model's own causal-LM cross-entropy (`outputs.loss`: ONE
    mean over the label rows of the whole micro-batch), micro-batch means averaged over an accumulation window and over the ranks (a mean of
    means, as HF does - not token-weighted).  The loop itself (VLTrainerLoop) is VLDPOTrainer's."""

    def __init__(
        self,
        model=None,
        args=None,
        data_collator: Any = None,
        train_dataset=None,
        eval_dataset=None,
        processor=None,
        model_init: Optional[Callable] = None,
        compute_metrics: Optional[Callable] = None,
        callbacks: Optional[List] = None,
        optimizers: Tuple = (None, None),
        preprocess_logits_for_metrics: Optional[Callable] = None,
        peft_config: Optional[Dict] = None,
        dataset_text_field: Optional[str] = None,
        packing: Optional[bool] = True,
        formatting_func: Optional[Callable] = None,
        max_seq_length: Optional[int] = None,
        infinite: Optional[bool] = None,
        num_of_sequences: Optional[int] = 1024,
        chars_per_token: Optional[float] = 3.6,
        dataset_num_proc: Optional[int] = None,
        dataset_batch_size: int = 1000,
        neftune_noise_alpha: Optional[float] = None,
        model_init_kwargs: Optional[Dict] = None,
        dataset_kwargs: Optional[Dict] = None,
        eval_packing: Optional[bool] = None,
    ):
        # argument order = reference base/trainer.py:574-601
        if model is None:
            raise ValueError("VLSFTTrainer needs a model")
        self._init_neftune(model, args, neftune_noise_alpha)
        if peft_config is not None:          # trl SFTTrainer.__init__: model = get_peft_model(model, peft_config)
            if not hasattr(model, "apply_lora"):
                raise ValueError("peft_config given but the model wrapper has no apply_lora()")
            model.apply_lora(peft_config)
        self.is_peft_model = bool(getattr(model, "is_peft_model", False))
        self.processor = processor
        self.tokenizer = processor.tokenizer if processor is not None else None
        self.model = model
        self.args = args
        # trl: max_seq_length None -> min(tokenizer.model_max_length, 1024)
        self.max_seq_length = max_seq_length if max_seq_length is not None else min(int(getattr(self.tokenizer, "model_max_length", 1024) or 1024), 1024)
        self.dataset_text_field = dataset_text_field
        self.packing = packing               # accepted and ignored: the reference's _prepare_dataset override (:656-674) never packs
        self.dataset_num_proc = dataset_num_proc
        self.callbacks = list(callbacks or [])
        self._stored_metrics = defaultdict(lambda: defaultdict(list))
        self.log_history: List[dict] = []
        self.accelerator = _Accelerator(model)
        self.data_collator = data_collator
        self.train_dataset = self._prepare_dataset(train_dataset)
        self.eval_dataset = self._prepare_dataset(eval_dataset)
        self.state = _State()

    # ------------------------------------------------------------------------------------------ tokenisation
    def tokenize_row(self, element):
        """reference :631-654, quirk included: every eos INSIDE the conversation gets attention_mask 0 and label -100 (a hole in the
        middle of the key mask), then one eos is appended with mask 1 and label eos, then everything is cut to max_seq_length."""
        conv = element["conversations"]
        image = element["img_path"]
        first_sentence = conv[0]["value"]
        first_sentence = self.processor.format_multimodal_prompt(first_sentence, image)
        conv[0]["value"] = first_sentence
        tokens = self.processor.process_batch_conv([conv])["full"]  # process_batch_conv adds bos token but no eos token
        tokens = {k: v[0] for k, v in tokens.items()}
        eos = self.tokenizer.eos_token_id
        eos_indices = {i for i, x in enumerate(tokens["input_ids"]) if x == eos}
        tokens["attention_mask"] = [0 if i in eos_indices else m for i, m in enumerate(tokens["attention_mask"])]
        tokens["labels"] = [-100 if i in eos_indices else l for i, l in enumerate(tokens["labels"])]
        tokens["input_ids"] = list(tokens["input_ids"]) + [eos]
        tokens["attention_mask"] = tokens["attention_mask"] + [1]
        tokens["labels"] = tokens["labels"] + [eos]
        tokens = {k: v[: self.max_seq_length] for k, v in tokens.items()}
        tokens["img_path"] = image
        return tokens

    def _prepare_dataset(self, dataset, *unused, **unused_kw):
        """reference :656-674: every row through tokenize_row, only input_ids / labels / attention_mask / img_path kept; no packing.
        Rows that already carry input_ids (pre-tokenised) pass through."""
        if dataset is None:
            return None
        rows = list(dataset)
        if rows and "input_ids" not in rows[0]:
            rows = [self.tokenize_row({k: (copy.deepcopy(v) if k == "conversations" else v) for k, v in dict(r).items()}) for r in rows]
        keep = ("input_ids", "labels", "attention_mask", "img_path")
        return [{k: r[k] for k in keep if k in r} for r in rows]

    # ------------------------------------------------------------------------------------------ loss
    def compute_loss(self, model, inputs, return_outputs: bool = False):
        """transformers Trainer.compute_loss: outputs = model(**inputs); loss = outputs["loss"] - the cross-entropy the wrapper computes on
        the fused lm-head when `loss` is read (LlavaForRL.causal_lm_loss)."""
        outputs = model(**{k: v for k, v in inputs.items() if k != "img_path"})
        loss = model.causal_lm_loss(outputs) if hasattr(model, "causal_lm_loss") else outputs["loss"]
        if loss is None:
            raise ValueError("The model did not return a loss from the inputs, only the following keys: "
                             f"{','.join(k for k in inputs.keys())}.")
        return (loss, outputs) if return_outputs else loss

    def prediction_step(self, model, inputs, prediction_loss_only: bool = True, ignore_keys=None):
        with torch.no_grad():
            loss, outputs = self.compute_loss(model, self._prepare_inputs(inputs), return_outputs=True)
        if prediction_loss_only:
            return loss.detach(), None, None
        return loss.detach(), outputs.logits, outputs.labels


class VLRMTrainer(VLTrainerLoop):
    """Reward-model training - mirror of the reference src/vlrlhf/base/trainer.py:502-570 plus what it inherits from trl==0.8.1
    `RewardTrainer` on this path: loss = -logsigmoid(r_chosen - r_rejected).mean() (compute_loss), eval accuracy = the share of pairs
    whose chosen reward is not below the rejected one (compute_accuracy: argmax over [r_chosen, r_rejected], ties to the first).

    The reference runs chosen and rejected as two forwards, each padded to its own width, and reads every reward at the last column of
    its batch.  Here both halves are ONE concatenated pass (as VLDPOTrainer.concatenated_forward: right-padded to the wider half, images
    shared through `_vlr_dup`), each sequence's reward read at the last column of ITS OWN half: under right padding and causal
    key-masked attention that row does not depend on the columns behind it, so the values are those of the two passes.  The pair loss
    is vlr_dpo_loss with beta 1 and reference_free (the two reference arrays are zeros).  Deliberate difference: `img_path` is kept by
    tokenize_row and images reach the model as they do in DPO.  NEFTune stays off on this path."""

    def __init__(
        self,
        model=None,
        args=None,
        data_collator: Any = None,
        train_dataset=None,
        eval_dataset=None,
        processor=None,
        model_init: Optional[Callable] = None,
        compute_metrics: Optional[Callable] = None,
        callbacks: Optional[List] = None,
        optimizers: Tuple = (None, None),
        preprocess_logits_for_metrics: Optional[Callable] = None,
        max_length: Optional[int] = None,
        peft_config: Optional[Dict] = None,
    ):
        # argument order = reference base/trainer.py:503-518
        if model is None:
            raise ValueError("VLRMTrainer needs a model")
        if not hasattr(model, "reward_rows"):
            raise ValueError("VLRMTrainer needs a reward model (vlrlhf.base.model.VLRewardModel)")
        if peft_config is not None:          # trl RewardTrainer.__init__: model = get_peft_model(model, peft_config)
            model.apply_lora(peft_config)
        self.is_peft_model = bool(getattr(model, "is_peft_model", False))
        self.processor = processor
        self.tokenizer = processor.tokenizer if processor is not None else None
        self.model = model
        self.args = args
        self.max_length = max_length
        pad = getattr(data_collator, "pad_token_id", None)
        if pad is None and self.tokenizer is not None:
            pad = self.tokenizer.pad_token_id
        self.padding_value = int(pad) if pad is not None else 0
        self.callbacks = list(callbacks or [])
        self.use_reward_data_collator = True
        self._stored_metrics = defaultdict(lambda: defaultdict(list))
        self.log_history: List[dict] = []
        self.accelerator = _Accelerator(model)
        self.data_collator = data_collator
        self.train_dataset = self._tokenize_dataset(train_dataset)
        self.eval_dataset = self._tokenize_dataset(eval_dataset)
        self.state = _State()

    # ------------------------------------------------------------------------------------------ tokenisation
    def _tokenize_dataset(self, ds):
        if ds is None:
            return None
        rows = list(ds)
        if rows and "input_ids_chosen" not in rows[0]:
            rows = [self.tokenize_row(dict(r)) for r in rows]
        return rows

    def tokenize_row(self, element):
        """reference :550-570, plus `img_path`"""
        prompt = self.processor.format_multimodal_prompt(element["prompt"], element["img_path"])
        out = {}
        for side in ("chosen", "rejected"):
            conv = self.processor.make_single_turn_conv(prompt, element[side])
            full = self.processor.process_batch_conv([conv])["full"]
            out[f"input_ids_{side}"] = full["input_ids"][0][: self.max_length]
            out[f"attention_mask_{side}"] = full["attention_mask"][0][: self.max_length]
        out["img_path"] = element["img_path"]
        return out

    # ------------------------------------------------------------------------------------------ loss
    def concatenated_inputs(self, batch) -> Dict[str, Any]:
        """[chosen ; rejected] right-padded to the wider half, every image input doubled (`_vlr_dup = 2`: the frozen tower sees each
        distinct image once), and `reward_cols`: the last TOKEN column of each sequence's own half.  Memoised on the batch."""
        src = tuple(id(batch.get(k)) for k in ("input_ids_chosen", "input_ids_rejected", "attention_mask_chosen",
                                               "attention_mask_rejected", "img_input_dict"))
        cache = batch.get("_vlr_rm_concat")
        if cache is not None and cache["src"] == src:
            return cache["out"]
        dev = self.accelerator.device
        ic, ir = batch["input_ids_chosen"], batch["input_ids_rejected"]
        if ic.shape[0] != ir.shape[0]:
            raise ValueError(f"{ic.shape[0]} chosen rows but {ir.shape[0]} rejected rows")
        n = max(ic.shape[1], ir.shape[1])
        ids = torch.cat([pad_to_length(ic, n, self.padding_value), pad_to_length(ir, n, self.padding_value)], dim=0).to(dev)
        mask = torch.cat([pad_to_length(batch["attention_mask_chosen"], n, 0), pad_to_length(batch["attention_mask_rejected"], n, 0)], dim=0).to(dev)
        ids._vlr_meta = {}
        img = {}
        for k, v in (batch.get("img_input_dict") or {}).items():
            if isinstance(v, torch.Tensor):
                t = torch.cat([v, v], dim=0).to(dev)
                t._vlr_dup = 2
                img[k] = t
            elif isinstance(v, list):
                img[k] = v + v
            else:
                raise ValueError(f"Unsupported type {type(v)} for concatenation.")
        B = ic.shape[0]
        out = dict(input_ids=ids, attention_mask=mask, img=img, pairs=B,
                   reward_cols=torch.tensor([ic.shape[1] - 1] * B + [ir.shape[1] - 1] * B, dtype=torch.int64))
        batch["_vlr_rm_concat"] = dict(src=src, out=out)
        return out

    def concatenated_forward(self, model, batch):
        """-> (rewards_chosen [B], rewards_rejected [B]) fp32 from one pass over [chosen ; rejected]"""
        cb = self.concatenated_inputs(batch)
        rewards = model(input_ids=cb["input_ids"], attention_mask=cb["attention_mask"], reward_cols=cb["reward_cols"], **cb["img"])[0]
        rewards = rewards.squeeze(-1)
        return rewards[: cb["pairs"]], rewards[cb["pairs"]:]

    def pair_loss(self, rewards_chosen, rewards_rejected):
        """-logsigmoid(r_chosen - r_rejected) per pair, forward and backward in vlr_dpo_loss (beta 1, reference_free)"""
        zeros = torch.zeros_like(rewards_chosen)
        losses, _, _ = _DpoLossFn.apply(rewards_chosen, rewards_rejected, zeros, zeros, 1.0, 0.0, 0, 1)
        return losses

    def compute_loss(self, model, inputs, return_outputs: bool = False):
        """trl==0.8.1 RewardTrainer.compute_loss (no margin column in this pipeline)"""
        rc, rr = self.concatenated_forward(model, inputs)
        loss = self.pair_loss(rc, rr).mean()
        if return_outputs:
            return loss, {"rewards_chosen": rc, "rewards_rejected": rr}
        return loss

    def prediction_step(self, model, inputs, prediction_loss_only: bool = False, ignore_keys=None):
        """trl RewardTrainer.prediction_step + compute_accuracy: every pair adds 1 to eval_accuracy when r_chosen >= r_rejected (numpy
        argmax takes the first of two equal logits, so a tie counts as correct); -> (loss, logits [B, 2], labels = zeros)"""
        with torch.no_grad():
            loss, out = self.compute_loss(model, self._prepare_inputs(inputs), return_outputs=True)
        rc, rr = out["rewards_chosen"].detach(), out["rewards_rejected"].detach()
        self._stored_metrics["eval"]["eval_accuracy"].extend((rc >= rr).float().unbind(0))
        if prediction_loss_only:
            return loss.detach(), None, None
        logits = torch.stack([rc, rr], dim=1).softmax(dim=1)
        return loss.detach(), logits, torch.zeros(logits.shape[0], device=logits.device)

    def load_checkpoint(self, path: str) -> dict:
        state = super().load_checkpoint(path)
        # the base wrapper's state dict does not hold the head.  With an optimizer state the head came back with the master copy
        # (load_optimizer_state), under LoRA load_adapter read rm_head.bin; what is left is a checkpoint of the weights alone
        if not self.is_peft_model and not os.path.isfile(os.path.join(path, "optimizer_master.safetensors")):
            self.model.load_rm_head(path)
        return state


# ----------------------------------------------------------------------------------------------------------
# KTO: Kahneman-Tversky Optimization on unpaired feedback (trl KTOTrainer; include/vlr.h "KTO")
# ----------------------------------------------------------------------------------------------------------
class _KtoLossFn(torch.autograd.Function):
    """trl KTOTrainer.kto_loss forward, statistics and gradient in ONE launch of vlr_kto_loss -> (loss, losses [n], rewards [n],
    stats [8], dpi [n] at upstream 1).  Only `pi` is differentiated: the reference and both KL inputs are constants (the KL baseline is detached in trl).  The
    kernel's gradient is taken at upstream 1 and scaled by the incoming gradient of `loss` in backward - the shared loop applies
    1 / gradient_accumulation_steps at the optimizer step, as it does for DPO and SFT."""

    @staticmethod
    def forward(ctx, pi, ref, label, pi_kl, ref_kl, beta, w_desirable, w_undesirable):
        n, m, dev = pi.shape[0], pi_kl.shape[0], pi.device
        a = [t.detach().float().contiguous() for t in (pi, ref, pi_kl, ref_kl)]
        lab = label.to(device=dev, dtype=torch.uint8).contiguous()
        losses, rewards, dpi = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
        stats = torch.empty(8, dtype=torch.float32, device=dev)
        _hip.call("vlr_kto_loss", a[0], a[1], lab, n, a[2], a[3], m, float(beta), float(w_desirable), float(w_undesirable), 1.0, losses,
                  rewards, dpi, stats)
        ctx.save_for_backward(dpi)
        loss = stats[0].clone()
        ctx.mark_non_differentiable(losses, rewards, stats, dpi)
        return loss, losses, rewards, stats, dpi

    @staticmethod
    def backward(ctx, g_loss, g_losses, g_rewards, g_stats, g_dpi):
        (dpi,) = ctx.saved_tensors
        return dpi * g_loss, None, None, None, None, None, None, None


@dataclasses.dataclass
class KTOConfig:
    """the fields of trl's KTOConfig that this path reads (same names, same defaults) on top of the training arguments the shared loop
    reads (vlrlhf/dpo.py TrainingArguments: same names, same defaults)."""
    beta: float = 0.1
    desirable_weight: float = 1.0
    undesirable_weight: float = 1.0
    max_length: Optional[int] = 512
    max_prompt_length: Optional[int] = 128
    precompute_ref_log_probs: bool = False
    output_dir: str = "output"
    per_device_train_batch_size: int = 4
    gradient_accumulation_steps: int = 1
    learning_rate: float = 1e-6
    weight_decay: float = 0.0
    adam_beta1: float = 0.9
    adam_beta2: float = 0.98
    adam_epsilon: float = 1e-6
    max_grad_norm: float = 1.0
    warmup_ratio: float = 0.03
    warmup_steps: int = 0
    lr_scheduler_type: str = "cosine"
    num_train_epochs: float = 1.0
    max_steps: int = -1
    logging_steps: int = 10
    seed: int = 42
    bf16: bool = True
    tf32: bool = True
    gradient_checkpointing: bool = False
    use_lora: bool = False
    use_flash_attention_2: bool = True
    dataset_num_proc: Optional[int] = 16
    project_name: Optional[str] = "VL-RLHF"
    group_name: Optional[str] = "llava-1.5-7b-kto"
    resume_from_checkpoint: Optional[bool] = None
    report_to: str = "none"
    run_name: str = "kto"
    save_strategy: str = "no"
    save_steps: int = 500
    save_total_limit: int = 1
    evaluation_strategy: str = "no"
    eval_strategy: Optional[str] = None
    eval_steps: int = 500
    per_device_eval_batch_size: int = 4
    dataloader_num_workers: int = 0
    dataloader_drop_last: bool = False
    dataloader_prefetch: int = 2
    remove_unused_columns: bool = False
    local_rank: int = 0
    neftune_noise_alpha: Optional[float] = None

    def __post_init__(self):
        for name in ("beta", "desirable_weight", "undesirable_weight"):
            v = getattr(self, name)
            if v is None or not math.isfinite(float(v)):
                raise ValueError(f"{name} ({v}) must be a finite number")
        if self.eval_strategy:
            self.evaluation_strategy = self.eval_strategy


class VLKTOTrainer(VLTrainerLoop):
    """KTO on unpaired rows {prompt, completion, label, img_path} - trl's KTOTrainer on the MI355X path.  A collated batch (base/collator.py
    VLKTODataCollatorWithPadding) is shaped like a DPO batch: `chosen_*` the B main rows, `rejected_*` their KL rows (prompt i and image
    i with the completion of row i - 1), so the reference side is VLDPOTrainer's own code: concatenated_forward / _reference_logps, the
    adapter-off pass under LoRA, a frozen copy otherwise, the row-compact reference pass wherever DPO gets it.  The policy runs ONE
    training pass over the B main rows and ONE no-grad pass over the B KL rows - never a 2B-row training pass whose backward would cost
    twice what is needed.  The loss is vlr_kto_loss (_KtoLossFn).

    Deliberate differences from trl: the no-grad KL pass runs in eval mode (no LoRA dropout on a pass nothing differentiates - the choice
    GRPO made for its no-grad passes); `kl` is this process's mean, not an average across ranks - and more than one rank is refused."""

    dpo_trainer_cls = None      # the family's DPO trainer: its tokenize_row tokenises prompt + one answer (set below / by the model packages)

    def __init__(self, model=None, ref_model=None, args: Optional[KTOConfig] = None, train_dataset=None, eval_dataset=None, processor=None,
                 data_collator: Any = None, peft_config: Optional[Dict] = None, label_pad_token_id: int = -100, padding_value: int = None,
                 truncation_mode: str = "keep_end", precompute_ref_log_probs: bool = False, reference_free: bool = False,
                 callbacks: Optional[List] = None, dataset_num_proc: Optional[int] = None):
        if model is None:
            raise ValueError("VLKTOTrainer needs a model")
        if args is None:
            args = KTOConfig()
        # ---- refused by name, before anything is built or changed
        if _world() > 1:
            raise NotImplementedError("KTO on more than one GPU: trl averages kl across the ranks, and that has never been run on the "
                                      "MI355X path")
        if precompute_ref_log_probs or getattr(args, "precompute_ref_log_probs", False):
            raise NotImplementedError("precompute_ref_log_probs: the KL rows change with the batch's composition, and the pre-pass that "
                                      "would store them per batch is not built")
        if reference_free:
            raise NotImplementedError("reference_free: KTO's rewards and its KL baseline are log-ratios against a reference model")
        if bool(getattr(model, "is_packed", False)):
            raise NotImplementedError("q_lora: KTO over a packed GPTQ base has never been run on the MI355X path")
        if bool(getattr(getattr(model, "engine", None), "train_vision", False)):
            raise NotImplementedError("--freeze_vision_tower False: KTO's two policy passes would both need the tower's backward state; "
                                      "the tower stays frozen on this path")
        if hasattr(model, "v_head"):
            raise ValueError("a model with a value head: KTO trains a plain family wrapper (LlavaForRL, QwenVLForRL), it has no value head")
        if int(getattr(args, "per_device_train_batch_size", 4)) < 2:
            from .collator import KTO_BATCH_OF_ONE
            raise ValueError(KTO_BATCH_OF_ONE)
        if peft_config is not None:
            if not hasattr(model, "apply_lora"):
                raise ValueError("peft_config given but the model wrapper has no apply_lora()")
            model.apply_lora(peft_config)
        self.is_peft_model = bool(getattr(model, "is_peft_model", False))
        self._init_neftune(model, args)
        self.processor = processor
        self.tokenizer = processor.tokenizer if processor is not None else None
        self.model = model
        self.args = args
        self.beta = float(args.beta)
        self.desirable_weight = float(args.desirable_weight)
        self.undesirable_weight = float(args.undesirable_weight)
        self.loss_type = "kto"
        self.label_pad_token_id = label_pad_token_id
        self.padding_value = padding_value if padding_value is not None else (
            self.tokenizer.pad_token_id if self.tokenizer is not None and self.tokenizer.pad_token_id is not None else 0)
        self.truncation_mode = truncation_mode
        self.max_length = args.max_length if getattr(args, "max_length", None) is not None else 512
        self.max_prompt_length = args.max_prompt_length if getattr(args, "max_prompt_length", None) is not None else 128
        self.max_target_length = None
        self.is_encoder_decoder = False
        self.dataset_num_proc = dataset_num_proc
        self.callbacks = list(callbacks or [])
        self._stored_metrics = defaultdict(lambda: defaultdict(list))
        self.log_history: List[dict] = []
        self.accelerator = _Accelerator(model)
        if ref_model is None and not self.is_peft_model:      # trl: no ref_model and no peft -> a frozen deep copy of the policy
            ref_model = model.create_reference_model() if hasattr(model, "create_reference_model") else None
        self.ref_model = ref_model
        self.data_collator = data_collator
        self.train_dataset = self._tokenize_dataset(train_dataset)
        self.eval_dataset = self._tokenize_dataset(eval_dataset)
        self.state = _State()
        self._warn_balance()

    # the reference side and the log-probs are VLDPOTrainer's own code on the [chosen ; rejected]-shaped batch
    build_tokenized_answer = VLDPOTrainer.build_tokenized_answer
    _trl_tokenize_row = VLDPOTrainer._trl_tokenize_row
    concatenated_inputs = VLDPOTrainer.concatenated_inputs
    get_batch_logps = staticmethod(VLDPOTrainer.get_batch_logps)
    concatenated_forward = VLDPOTrainer.concatenated_forward
    _reference_logps = VLDPOTrainer._reference_logps
    _reference_pass = staticmethod(VLDPOTrainer._reference_pass)
    null_ref_context = VLDPOTrainer.null_ref_context

    # ------------------------------------------------------------------------------------------ rows
    def _tokenize_dataset(self, ds):
        if ds is None:
            return None
        rows = list(ds)
        if rows and "completion_input_ids" not in rows[0]:
            rows = [self.tokenize_row(dict(r)) for r in rows]
        return rows

    def tokenize_row(self, feature, model=None) -> Dict:
        """prompt + one answer exactly as the family's DPO trainer tokenises a pair's chosen side (its tokenize_row on chosen = rejected =
        completion: the same template, split, truncation and labels, -100 on the prompt) -> completion_input_ids / _attention_mask /
        _labels, label, img_path"""
        cls = self.dpo_trainer_cls or VLDPOTrainer
        pair = cls.tokenize_row(self, dict(prompt=feature["prompt"], chosen=feature["completion"], rejected=feature["completion"],
                                           img_path=feature["img_path"]))
        out = {f"completion_{k}": pair[f"chosen_{k}"] for k in ("input_ids", "attention_mask", "labels")}
        out["label"] = bool(feature["label"])
        out["img_path"] = feature["img_path"]
        return out

    def _warn_balance(self):
        """trl's advice: desirable_weight n_desirable / (undesirable_weight n_undesirable) should lie in [1, 4/3]; one log line otherwise"""
        rows = self.train_dataset or []
        n_d = sum(1 for r in rows if r.get("label"))
        n_u = len(rows) - n_d
        self.balance_warning = None
        if n_d == 0 or n_u == 0 or self.undesirable_weight == 0:
            return
        ratio = self.desirable_weight * n_d / (self.undesirable_weight * n_u)
        if not 1.0 <= ratio <= 4.0 / 3.0:
            self.balance_warning = (f"[vlrlhf.kto] WARNING: desirable_weight * n_desirable / (undesirable_weight * n_undesirable) = "
                                    f"{self.desirable_weight:g} * {n_d} / ({self.undesirable_weight:g} * {n_u}) = {ratio:.3f} lies outside "
                                    f"[1, 4/3]; set the weights so that it lies inside (the KTO paper's advice for imbalanced data)")
            if _rank() == 0:
                print(self.balance_warning, flush=True)

    # a batch of one row has no KL row: a trailing batch of one is left out of the epoch (and of evaluate), and counted that way
    def _train_row_batches(self, epoch: int):
        for rows in super()._train_row_batches(epoch):
            if len(rows) >= 2:
                yield rows

    def _batches_per_epoch(self) -> int:
        n = super()._batches_per_epoch()
        bs = int(getattr(self.args, "per_device_train_batch_size", 4))
        per_rank = -(-len(self.train_dataset) // _world())
        if not getattr(self.args, "dataloader_drop_last", False) and per_rank % bs == 1:
            n -= 1      # (the batch left out is always the LAST of the epoch: a resumed run skips the same batches in front of it)
        return n

    def evaluate(self, eval_dataset=None, metric_key_prefix: str = "eval") -> Dict[str, float]:
        ds = list(eval_dataset if eval_dataset is not None else (self.eval_dataset or []))
        bs = int(getattr(self.args, "per_device_eval_batch_size", None) or getattr(self.args, "per_device_train_batch_size", 4))
        if bs < 2:
            from .collator import KTO_BATCH_OF_ONE
            raise ValueError(KTO_BATCH_OF_ONE.replace("per_device_train_batch_size", "per_device_eval_batch_size"))
        if len(ds) % bs == 1:
            if _rank() == 0:
                print(f"[vlrlhf.kto] evaluate: {len(ds)} rows in batches of {bs} leave a last batch of one row, which has no KL row: it is left out",
                      flush=True)
            ds = ds[:-1]
        return super().evaluate(ds, metric_key_prefix)

    # ------------------------------------------------------------------------------------------ the passes of a step
    def _half_logps(self, model, batch, half: str):
        """summed completion log-probs [B] of one half of the batch (`chosen`: the main rows, `rejected`: the KL rows) on a plain forward
        of those B rows with the batch's own images"""
        dev = self.accelerator.device
        labels = batch[f"{half}_labels"].to(dev)
        img = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in (batch.get("img_input_dict") or {}).items()}
        out = model(input_ids=batch[f"{half}_input_ids"].to(dev), attention_mask=batch[f"{half}_attention_mask"].to(dev), labels=labels,
                    use_cache=False, **img)
        final = out.labels if getattr(out, "labels", None) is not None else labels
        return self.get_batch_logps(out.logits, final, average_log_prob=False, label_pad_token_id=self.label_pad_token_id)

    def kto_loss(self, pi, ref, label, pi_kl, ref_kl):
        """-> (loss, losses [B], rewards [B], stats [8], dpi [B] at upstream 1) of vlr_kto_loss"""
        return _KtoLossFn.apply(pi, ref, label, pi_kl, ref_kl, self.beta, self.desirable_weight, self.undesirable_weight)

    def get_batch_loss_metrics(self, model, batch, train_eval: Literal["train", "eval"] = "train"):
        """reference log-probs of both halves (VLDPOTrainer._reference_logps), the policy's no-grad eval-mode pass over the KL rows, its
        pass over the main rows (a training pass under training_step), the loss"""
        if batch["chosen_input_ids"].shape[0] < 2:
            from .collator import KTO_BATCH_OF_ONE
            raise ValueError(KTO_BATCH_OF_ONE)
        ref, ref_kl = self._reference_logps(batch)
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                pi_kl = self._half_logps(model, batch, "rejected")
        finally:
            model.train(was_training)
        pi = self._half_logps(model, batch, "chosen")
        loss, losses, rewards, stats, dpi = self.kto_loss(pi, ref, batch["kto_label"], pi_kl, ref_kl)
        prefix = "eval_" if train_eval == "eval" else ""
        names = ("rewards/chosen_sum", "rewards/rejected_sum", "logps/chosen_sum", "logps/rejected_sum", "count/chosen", "count/rejected")
        metrics = {f"{prefix}{k}": stats[2 + i] for i, k in enumerate(names)}
        metrics[f"{prefix}kl"] = stats[1]
        if self.keep_last:
            self.last = dict(pi=pi.detach(), ref=ref, pi_kl=pi_kl, ref_kl=ref_kl, losses=losses, rewards=rewards, stats=stats, dpi=dpi)
        return loss, metrics

    keep_last = False      # tests: keep the log-probs of the last batch in `self.last`

    def compute_loss(self, model, inputs, return_outputs: bool = False):
        loss, metrics = self.get_batch_loss_metrics(model, inputs, train_eval="train")
        self.store_metrics(metrics, train_eval="train")
        if return_outputs:
            return loss, metrics
        return loss

    def prediction_step(self, model, inputs, prediction_loss_only: bool = True, ignore_keys=None):
        with torch.no_grad():
            loss, metrics = self.get_batch_loss_metrics(model, self._prepare_inputs(inputs), train_eval="eval")
        self.store_metrics(metrics, train_eval="eval")
        return loss.detach(), None, None


@dataclasses.dataclass
class PPOConfig:
    """the fields of trl==0.8.1 PPOConfig that the PPO step reads (same names, same defaults).  batch_size = the rows of one step(),
    backward_batch_size = mini_batch_size * gradient_accumulation_steps = the rows of one optimizer step."""
    learning_rate: float = 1.41e-5
    batch_size: int = 128
    mini_batch_size: int = 128
    gradient_accumulation_steps: int = 1
    ppo_epochs: int = 4
    gamma: float = 1.0
    lam: float = 0.95
    cliprange: float = 0.2
    cliprange_value: float = 0.2
    vf_coef: float = 0.1
    kl_penalty: str = "kl"
    init_kl_coef: float = 0.2
    adap_kl_ctrl: bool = True
    target: float = 6.0
    horizon: float = 10000.0
    whiten_rewards: bool = False
    ratio_threshold: float = 10.0
    early_stopping: bool = False
    target_kl: float = 1.0
    max_grad_norm: Optional[float] = None
    seed: int = 0
    world_size: int = 1
    # the reference's additions (src/vlrlhf/ppo.py PPOConfig) that this path reads
    use_lora: bool = False
    use_value_adapter: bool = False
    gradient_checkpointing: bool = False
    output_dir: Optional[str] = None
    per_device_gamelog_size: int = 2
    max_new_tokens: Optional[int] = None
    max_length: Optional[int] = None
    local_rank: int = -1
    # not in the reference: a checkpoint every save_steps steps of train() (0: none) and the one to resume from
    save_steps: int = 0
    resume_from_checkpoint: Optional[str] = None
    # trl's two entropy statistics (off: the step is launch for launch the one without them): "ppo/policy/entropy", the mean entropy of the
    # policy's softmax over the minibatch's response rows (from the lm-head pass the log-probs come from), and "objective/entropy", the mean
    # over the sequences of sum_t -old_logp_t.  No bonus: trl's PPO has none.
    log_entropy: bool = False
    # generate(sampler="device") with seed = config.seed + 2: one vlr_sample_tokens launch per token instead of the torch ops, the
    # generation config's temperature / top_k honoured, a counter-based draw whose call counter rides in the checkpoint (off: unchanged)
    device_sampler: bool = False

    def __post_init__(self):
        self.backward_batch_size = self.mini_batch_size * self.gradient_accumulation_steps
        if self.batch_size <= 0 or self.mini_batch_size <= 0 or self.batch_size % self.backward_batch_size:
            raise ValueError(f"batch_size ({self.batch_size}) must be a multiple of mini_batch_size * gradient_accumulation_steps "
                             f"({self.backward_batch_size})")
        if self.per_device_gamelog_size > self.batch_size:
            raise ValueError("per_device_gamelog_size should be less than batch_size")
        if self.use_value_adapter and not self.use_lora:
            raise ValueError("You can only use value adapter with a Peft base model. Please set use_lora to True.")
        if self.max_new_tokens is not None and self.max_length is not None:
            raise ValueError("You can only use one of max_new_tokens and max_length")
        if self.kl_penalty not in ("kl", "abs", "mse", "full"):
            raise ValueError(f"kl_penalty must be one of 'kl', 'abs', 'mse', 'full', got {self.kl_penalty!r}")


class AdaptiveKLController:
    """trl AdaptiveKLController: e = clip(kl / target - 1, -0.2, 0.2); value *= 1 + e * n_steps / horizon"""

    def __init__(self, init_kl_coef, target, horizon):
        self.value, self.target, self.horizon = float(init_kl_coef), float(target), float(horizon)

    def update(self, current, n_steps):
        e = min(max(current / self.target - 1.0, -0.2), 0.2)
        self.value *= 1.0 + e * n_steps / self.horizon


class FixedKLController:
    def __init__(self, kl_coef):
        self.value = float(kl_coef)

    def update(self, current, n_steps):
        pass


KL_PENALTY_IDS = {"kl": 0, "abs": 1, "mse": 2}


class VLOnlineRLTrainer:
    """What the online-RL trainers (VLPPOTrainer, VLGRPOTrainer) share: tokenize_row and the shuffled batches, scoring by a separate reward
    model, the logging seam, checkpoint / resume (weights, optimizer, the row order and whatever `_checkpoint_extra` adds), the
    [query ; response] batch with its image inputs, and sampling through the model's own generate.  A subclass sets config, model,
    reward_model, processor, tokenizer, data_collator, dataset, generation_kwargs, is_peft_model, accelerator, padding_value, state,
    log_history and _data_gen in its __init__ (`_init_shared`), and provides step() and train()."""

    IMAGE_KEYS = ("pixel_values",)      # what of a collated batch reaches the models as image input

    def _init_shared(self, config, model, reward_model, processor, dataset, data_collator, generation_kwargs):
        self.config, self.model, self.reward_model = config, model, reward_model
        self.processor, self.dataset, self.data_collator = processor, dataset, data_collator
        self.tokenizer = processor.tokenizer if processor is not None else None
        self.generation_kwargs = dict(generation_kwargs or {})
        self.is_peft_model = bool(getattr(model, "is_peft_model", False))
        self.accelerator = _Accelerator(model)
        pad = getattr(self.tokenizer, "pad_token_id", None)
        self.padding_value = int(pad) if pad is not None else 0
        self.state = _State()
        self.log_history: List[dict] = []
        self.dataset = self._tokenize_dataset(dataset)
        self._data_gen = torch.Generator().manual_seed(int(config.seed) + 1)      # the order of the rows, apart from the step's permutations
        self._epoch_data_state = self._data_gen.get_state().tolist()

    # ------------------------------------------------------------------------------------------ data
    def _tokenize_dataset(self, ds):
        if ds is None:
            return None
        rows = list(ds)
        if rows and "input_ids" not in rows[0]:
            rows = [self.tokenize_row(dict(r)) for r in rows]
        return rows

    def tokenize_row(self, element):
        """reference :416-426: the query with its image placeholder, as a single-turn conversation with an empty answer - the ids end
        where the assistant begins.  No labels.  The image travels as `img_path` (the key the collators read; the reference's `image`
        is accepted too)."""
        image = element["img_path"] if "img_path" in element else element["image"]
        query = self.processor.format_multimodal_prompt(element["query"], image)
        conv = self.processor.make_single_turn_conv(query, "")
        tokens = self.processor.process_batch_conv([conv])["full"]
        tokens = {k: v[0] for k, v in tokens.items() if k != "labels"}
        tokens["query"] = query
        tokens["img_path"] = image
        return tokens

    def get_batches(self):
        """one pass over the dataset: shuffled rows in batches of config.batch_size through the collator, the last partial batch dropped
        (trl prepare_dataloader: shuffle=True, drop_last=True)"""
        n, bs = len(self.dataset), self.config.batch_size
        self._epoch_data_state = self._data_gen.get_state().tolist()      # a checkpoint restores the generator to where this pass began
        order = torch.randperm(n, generator=self._data_gen).tolist()
        for lo in range(0, n - bs + 1, bs):
            yield self.data_collator([self.dataset[i] for i in order[lo:lo + bs]])

    # ------------------------------------------------------------------------------------------ scoring
    def compute_scores(self, queries_text, responses_text, img):
        """the separate reward model on the rebuilt conversations -> scores [n] fp32.  Deliberate difference from the reference, which
        left-pads and reads column -1: rows are right-padded and every row's reward is read at its own last token (reward_cols), the
        path VLRewardModel's tests cover; the rows of a batch must carry the same number of images (VLRewardModel's rule)."""
        if self.reward_model is None:
            raise NotImplementedError("scoring needs a separate reward_model (VLRewardModel); a reward adapter on the policy's base is not "
                                      "built on the MI355X path")
        convs = [self.processor.make_single_turn_conv(q, r) for q, r in zip(queries_text, responses_text)]
        full = self.processor.process_batch_conv(convs)["full"]
        lens = [len(x) for x in full["input_ids"]]
        T = max(lens)
        ids = torch.full((len(lens), T), self.padding_value, dtype=torch.long)
        mask = torch.zeros(len(lens), T, dtype=torch.long)
        for i, (x, m) in enumerate(zip(full["input_ids"], full["attention_mask"])):
            ids[i, :lens[i]] = torch.as_tensor(x, dtype=torch.long)
            mask[i, :lens[i]] = torch.as_tensor(m, dtype=torch.long)
        dev = self.reward_model.engine.dev
        img = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in img.items()}
        return self.reward_model.score(ids.to(dev), mask.to(dev), reward_cols=torch.tensor([n - 1 for n in lens]), **img).float().cpu()

    def _checkpoint_extra(self):
        """what the trainer adds to trainer_state.json (JSON-ready)"""
        return {}

    def _sampling_model(self):
        """the model whose generate samples (under a value head: the wrapped one), which owns the device sampler's call counter"""
        return getattr(self.model, "pretrained_model", self.model)

    def _device_sampler_kwargs(self, kw):
        """config.device_sampler: generate's keywords for the device sampler, unless the caller set them"""
        if getattr(getattr(self, "config", None), "device_sampler", False):
            kw.setdefault("sampler", "device")
            kw.setdefault("seed", int(self.config.seed) + 2)
        return kw

    def _sampler_state(self):
        """the device sampler's part of the checkpoint: the count of sampled generate calls (the `call` word of its RNG counter)"""
        if not getattr(self.config, "device_sampler", False):
            return {}
        return dict(sampler_calls=int(getattr(self._sampling_model(), "_sampler_calls", 0)))

    def _restore_sampler_state(self, state):
        if "sampler_calls" in state:
            self._sampling_model()._sampler_calls = int(state["sampler_calls"])

    def _restore_extra(self, state, path):
        """the inverse of _checkpoint_extra, after the weights are loaded and before the optimizer state is"""

    def log(self, logs):
        """the logging seam of the other trainers: one entry per step in log_history, printed on rank 0"""
        logs = dict(logs, step=self.state.global_step)
        self.log_history.append(logs)
        if _rank() == 0:
            print({k: (round(v, 6) if isinstance(v, float) else v) for k, v in logs.items() if k != "game_log"}, flush=True)
        return logs

    # ------------------------------------------------------------------------------------------ checkpoints
    def save_checkpoint(self, path=None):
        """`output_dir/checkpoint-<step>/`: the weights (the adapter under LoRA, else the checkpoint; a value-head model adds its head
        to either), the optimizer state (fp32 master / m / v + step), and trainer_state.json with the step counter, the state of the
        row-order generator, the batches consumed, the log history and the trainer's own `_checkpoint_extra` (PPO: kl_coef and the
        permutation generator; GRPO: the sampling generator).  A directory is complete or absent."""
        import json
        import shutil
        from safetensors.torch import save_file
        eng = self.model.engine
        path = path or os.path.join(str(self.config.output_dir or "output"), f"checkpoint-{self.state.global_step}")
        tmp = path + ".tmp"
        shutil.rmtree(tmp, ignore_errors=True)
        os.makedirs(tmp)
        if self.is_peft_model:      # (VLModelWithValueHead.save_pretrained does the same under LoRA, and adds its head)
            self.model.save_adapter(tmp)
        else:
            self.model.save_pretrained(tmp)
        st = eng.optimizer_state()
        if st is not None:
            for k in ("master", "m", "v"):
                save_file({k: st[k].detach().cpu()}, os.path.join(tmp, f"optimizer_{k}.safetensors"))
        hist = [{k: v for k, v in h.items()} for h in self.log_history]
        with open(os.path.join(tmp, "trainer_state.json"), "w") as f:
            json.dump(dict(global_step=self.state.global_step, opt_step=eng.opt_step, data_generator_start=self._epoch_data_state,
                           batches_seen=int(getattr(self, "batches_seen", 0)), lora_calls=getattr(eng, "_lora_calls", 0),
                           batch_size=self.config.batch_size, log_history=hist, **self._checkpoint_extra()), f)
        shutil.rmtree(path, ignore_errors=True)
        os.replace(tmp, path)
        return path

    def load_checkpoint(self, path):
        """weights, optimizer, the row order and the trainer's own `_restore_extra` of a save_checkpoint directory -> its state dict"""
        import json
        from safetensors.torch import load_file
        eng = self.model.engine
        with open(os.path.join(path, "trainer_state.json")) as f:
            state = json.load(f)
        if int(state.get("batch_size", self.config.batch_size)) != self.config.batch_size:
            raise ValueError(f"resume_from_checkpoint: {path} was written with batch_size={state['batch_size']}, this run has {self.config.batch_size}")
        if self.is_peft_model:
            self.model.load_adapter(path)
        else:
            sd = {}
            for fn in sorted(os.listdir(path)):
                if fn.startswith("model") and fn.endswith(".safetensors"):
                    sd.update(load_file(os.path.join(path, fn)))
            eng.policy.load_state_dict(sd)
        self._restore_extra(state, path)
        if os.path.isfile(os.path.join(path, "optimizer_master.safetensors")):      # (the master copy carries the head too)
            bufs = {k: load_file(os.path.join(path, f"optimizer_{k}.safetensors"))[k] for k in ("master", "m", "v")}
            eng.load_optimizer_state(bufs["master"], bufs["m"], bufs["v"], state["opt_step"])
        if hasattr(eng, "_lora_calls"):
            eng._lora_calls = int(state.get("lora_calls", 0))
        self._data_gen.set_state(torch.tensor(state["data_generator_start"], dtype=torch.uint8))
        self.state.global_step = int(state["global_step"])
        self.log_history = list(state.get("log_history", []))
        return state

    # ------------------------------------------------------------------------------------------ batch
    def _build_batch(self, queries, responses):
        """[query ; response] right-padded; labels -100 except on the response tokens (every one counts, the first EOS included)"""
        n = len(queries)
        T = max(int(q.numel() + r.numel()) for q, r in zip(queries, responses))
        ids = torch.full((n, T), self.padding_value, dtype=torch.long)
        mask = torch.zeros(n, T, dtype=torch.long)
        labels = torch.full((n, T), -100, dtype=torch.long)
        for i, (q, r) in enumerate(zip(queries, responses)):
            q, r = q.reshape(-1).cpu().long(), r.reshape(-1).cpu().long()
            if r.numel() == 0:
                raise ValueError(f"step: response {i} is empty")
            L = q.numel() + r.numel()
            ids[i, :L] = torch.cat([q, r])
            mask[i, :L] = 1
            labels[i, q.numel():L] = r
        return ids, mask, labels

    def _rows_images(self, ids, img, rows):
        """the image inputs of the batch rows `rows` (in that order).  A tensor has one entry per IMAGE and is cut by the rows' image counts
        (the ids name them: the model's image_count_key).  A list has one entry per image or one per row, told apart by its length; where
        both lengths coincide while the rows carry unequal numbers of images the two readings differ, and the list is refused."""
        if not img:
            return {}
        n = ids.shape[0]
        tok = int(self.model.engine.cfg[self.model.image_count_key])
        cnt = (ids == tok).sum(-1).tolist()
        off = [0]
        for c in cnt:
            off.append(off[-1] + c)
        total = off[-1]
        by_image = [j for r in rows for j in range(off[r], off[r + 1])]
        out = {}
        for k, v in img.items():
            if isinstance(v, torch.Tensor):
                if len(v) != total:
                    raise ValueError(f"step: image input {k!r} has {len(v)} entries for {n} rows carrying {total} images")
                out[k] = v[torch.tensor(by_image, dtype=torch.long)].to(self.accelerator.device)
                continue
            if len(v) == total == n and any(c != 1 for c in cnt):
                raise ValueError(f"step: image input {k!r} has {len(v)} entries, which is both the number of rows and of images while the rows "
                                 f"carry {cnt} images: per row or per image cannot be told apart - pass a tensor, or one list per row")
            if len(v) == total:
                out[k] = [v[j] for j in by_image]
            elif len(v) == n:
                out[k] = [v[r] for r in rows]
            else:
                raise ValueError(f"step: image input {k!r} has {len(v)} entries for {n} rows carrying {total} images")
        return out

    # ------------------------------------------------------------------------------------------ sampling
    @torch.no_grad()
    def generate(self, queries, return_prompt: bool = False, generation_kwargs=None, batch_size=None, **img):
        """trl PPOTrainer.generate on a batch, as the reference's train() calls it: the queries (1-D id tensors) are LEFT-padded, the
        model's own `generate` samples with the image inputs and `self.generation_kwargs` (updated by `generation_kwargs`), and each row
        comes back without its prompt (unless return_prompt) and without what follows its first stop: an id of `eos_token_id`, or the last
        token of a `stop_words_ids` sequence of the generation config - the rules `generate` itself ends a row by.  The stop stays in the
        response (every response token counts in step(), the first EOS included).  Under LoRA the adapters run live (merge_lora=False).
        batch_size (trl's _generate_batched; the reference's train() passes 32): None samples all queries in one call; an integer k
        samples them k at a time, in order - each chunk left-padded to ITS longest query, each image input that has one entry per
        query (a tensor's first dimension, a list) sliced to the chunk's rows - and returns the responses in the queries' order."""
        kw = dict(self.generation_kwargs)
        kw.update(generation_kwargs or {})
        if self.is_peft_model:
            kw.setdefault("merge_lora", False)
        VLOnlineRLTrainer._device_sampler_kwargs(self, kw)
        queries = [q.reshape(-1).cpu().long() for q in queries]
        n = len(queries)
        if batch_size is None or int(batch_size) >= n:
            return self._generate_rows(queries, return_prompt, kw, img)
        if int(batch_size) < 1:
            raise ValueError(f"generate: batch_size must be a positive integer, got {batch_size}")
        responses = []
        for lo in range(0, n, int(batch_size)):
            hi = min(n, lo + int(batch_size))
            part = {k: (v[lo:hi] if (isinstance(v, torch.Tensor) and v.dim() >= 1 and v.shape[0] == n) or
                        (isinstance(v, (list, tuple)) and len(v) == n) else v) for k, v in img.items()}
            responses += self._generate_rows(queries[lo:hi], return_prompt, kw, part)
        return responses

    @staticmethod
    def _stop_rules(model, kw):
        """(eos ids, stop-word id sequences) that end a row of `model` under the generation keywords `kw`, as its generate reads them"""
        from ..models.Llava import stop_sequences
        gc = kw.get("generation_config")
        eos = kw.get("eos_token_id")
        if eos is None:
            eos = getattr(gc, "eos_token_id", None)
        if eos is None:
            eos = model.config.get("eos_token_id", 2)
        eos = set(eos) if isinstance(eos, (list, tuple)) else {int(eos)}
        stops = [t.cpu().tolist() for t in stop_sequences(getattr(gc, "stop_words_ids", None), "cpu")]
        return eos, stops

    def _generate_rows(self, queries, return_prompt, kw, img, fanout=1):
        """one call of the model's generate on `queries` (cpu id rows), left-padded to the longest -> the responses, cut at their stop.
        fanout = the num_return_sequences of `kw`: generate returns fanout rows per query, row p * fanout + j continuing query p"""
        n, T0, dev = len(queries), max(int(q.numel()) for q in queries), self.accelerator.device
        ids = torch.full((n, T0), self.padding_value, dtype=torch.long)
        mask = torch.zeros(n, T0, dtype=torch.long)
        for i, q in enumerate(queries):
            ids[i, T0 - q.numel():] = q
            mask[i, T0 - q.numel():] = 1
        img = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in img.items()}
        out = self.model.generate(input_ids=ids.to(dev), attention_mask=mask.to(dev), **kw, **img)
        gen = out[:, T0:].cpu()
        eos, stops = VLOnlineRLTrainer._stop_rules(self.model, kw)
        responses = []
        for i in range(n * fanout):
            row, end = gen[i].tolist(), gen.shape[1]
            for t, tok in enumerate(row):
                if tok in eos or any(len(sq) <= t + 1 and row[t + 1 - len(sq): t + 1] == sq for sq in stops):
                    end = t + 1
                    break
            r = gen[i, :end].clone()
            responses.append(torch.cat([queries[i // fanout], r]) if return_prompt else r)
        return responses


def sequence_neg_logp_mean(old_logp, seq_off):
    """trl's "objective/entropy" (record_step_stats): the mean over the sequences of sum_t -old_logp_t, in fp64 on the host"""
    x = old_logp.detach().double().cpu()
    return sum(-float(x[seq_off[s]:seq_off[s + 1]].sum()) for s in range(len(seq_off) - 1)) / (len(seq_off) - 1)


class VLPPOTrainer(VLOnlineRLTrainer):
    """The PPO optimisation step - trl==0.8.1 PPOTrainer.step as the reference's VLPPOTrainer (base/trainer.py) drives it, restated in
    include/vlr.h ("PPO") and run on the HIP engine: no-grad rollout passes of the policy (log-probs, values) and of the reference
    (the adapters switched off under LoRA, else a frozen copy made when none is given), rewards + GAE + whitening in
    vlr_ppo_advantages, then ppo_epochs x minibatches of forward, vlr_ppo_loss, backward and one Adam step per backward batch.

    tokenize_row, generate, scoring by a separate reward model, step, the train() loop and checkpoint / resume (weights, optimizer, kl_coef,
    the permutation generator and the row order) are here; the entry point is vlrlhf/ppo.py.

    Deliberate differences from trl: the image inputs reach every forward of the step (trl's prepare_model_inputs drops them); the
    entropy statistics are opt-in (PPOConfig.log_entropy: the pass over the vocabulary rides in the lm-head's epilogue); rollout and
    reference passes run in eval mode (no adapter dropout, no NEFTune noise); world_size > 1 is refused, since whitening and the KL mean are per process in trl
    and nothing here settles what they should be across ranks."""

    def __init__(self, config=None, model=None, ref_model=None, reward_model=None, processor=None, dataset=None, data_collator=None,
                 generation_kwargs=None):
        # argument order = the reference's VLPPOTrainer
        if config is None or model is None:
            raise ValueError("VLPPOTrainer needs a config and a model")
        if not hasattr(model, "v_head"):
            raise ValueError("VLPPOTrainer needs a model with a value head (vlrlhf.base.model.VLModelWithValueHead)")
        if int(getattr(config, "world_size", 1) or 1) > 1 or _world() > 1:
            raise NotImplementedError("PPO on more than one GPU: whitening and the KL mean are per process in trl and the MI355X path "
                                      "does not settle what they are across ranks")
        if config.kl_penalty == "full":
            raise NotImplementedError("kl_penalty='full' needs the [R][V] logits of the policy and the reference; 'kl', 'abs' and 'mse' are built")
        self._init_shared(config, model, reward_model, processor, dataset, data_collator, generation_kwargs)
        if ref_model is None and not self.is_peft_model:      # trl: create_reference_model(model) when none is given
            ref_model = model.pretrained_model.create_reference_model()
        self.ref_model = ref_model
        self.kl_ctl = (AdaptiveKLController(config.init_kl_coef, config.target, config.horizon) if config.adap_kl_ctrl
                       else FixedKLController(config.init_kl_coef))
        self._perm_gen = torch.Generator().manual_seed(int(config.seed))
        self._stored_metrics = defaultdict(lambda: defaultdict(list))
        self.time_phases = False      # tools/ppo_bench.py: HIP events around the rollout and the optimisation of step() -> last_timing
        self.keep_rollout = False     # True: step() leaves its rollout tensors in last_rollout (diagnostics, the tests); off, nothing outlives the step
        self.last_rollout = None
        model.engine.init_optimizer()

    def _checkpoint_extra(self):
        return dict(kl_coef=float(self.kl_ctl.value), perm_generator=self._perm_gen.get_state().tolist(), **self._sampler_state())

    def _restore_extra(self, state, path):
        if not self.is_peft_model:      # (under LoRA load_adapter has read the head)
            self.model.load_v_head(path)
        self.kl_ctl.value = float(state["kl_coef"])
        self._perm_gen.set_state(torch.tensor(state["perm_generator"], dtype=torch.uint8))
        self._restore_sampler_state(state)

    # ------------------------------------------------------------------------------------------ loop
    def train(self, resume_from_checkpoint=None):
        """reference :428-499: per batch - generate, decode, rebuild the conversations, score with the reward model, step, log (the
        `log` seam; no wandb tables: the per_device_gamelog_size first rows are logged as text).  A batch whose scoring raises is
        skipped.  config.save_steps > 0 writes a checkpoint every so many steps; resume_from_checkpoint continues one."""
        resume = resume_from_checkpoint or getattr(self.config, "resume_from_checkpoint", None)
        skip = 0
        if resume:
            skip = int(self.load_checkpoint(resume).get("batches_seen", 0))
        self.batches_seen = 0
        for batch in self.get_batches():
            self.batches_seen += 1
            if self.batches_seen <= skip:      # the rows a resumed run has already consumed (the row order is part of the checkpoint)
                continue
            queries = batch["input_ids"]
            img = {k: batch[k] for k in self.IMAGE_KEYS if k in batch}
            responses = self.generate(queries, return_prompt=False, batch_size=32, **img)      # reference :437-442
            batch["response"] = self.tokenizer.batch_decode(responses, skip_special_tokens=True)
            try:
                scores = self.compute_scores(batch["query"], batch["response"], img)
            except NotImplementedError:
                raise
            except Exception as e:      # reference: warn, print the responses, skip the batch
                print(f"[ppo] WARNING: error when computing reward score, skipping this batch: {e!r}\n{batch['response']}", flush=True)
                self.skipped_batches = getattr(self, "skipped_batches", 0) + 1
                continue
            stats = self.step(queries, responses, [float(x) for x in scores], **img)
            k = self.config.per_device_gamelog_size
            game = [dict(query=self.processor.remove_image_placeholder(q), response=r, reward=float(s))
                    for q, r, s in zip(batch["query"][:k], batch["response"][:k], scores[:k])]
            self.log(dict(stats, game_log=game))
            if self.config.save_steps and self.state.global_step % self.config.save_steps == 0:
                self.save_checkpoint()
        return self.log_history

    def _reference_logps(self, ids, mask, labels, img):
        """token log-probs [R] of the reference on the response rows, under no-grad"""
        dev = self.accelerator.device
        if self.ref_model is None:
            with self.model.disable_adapter():
                return self.model(ids.to(dev), mask.to(dev), labels.to(dev), **img)[0]
        if hasattr(self.ref_model, "v_head"):
            return self.ref_model(ids.to(dev), mask.to(dev), labels.to(dev), **img)[0]
        out = self.ref_model(input_ids=ids.to(dev), attention_mask=mask.to(dev), labels=labels.to(dev), **img)
        c = out.logits.c
        return self.ref_model.engine.logps_forward(c, c["labels"], None, False, -100, reduce_seq=False)[1]["tok"]

    # ------------------------------------------------------------------------------------------ step
    def step(self, queries, responses, scores, **img):
        """one PPO optimisation step over config.batch_size (query, response, score) triples -> the stats dict under trl's key names.
        `img`: the batch's image inputs as the model's forward takes them (pixel_values / img_path ...); they reach every pass."""
        cfg, model, eng, dev = self.config, self.model, self.model.engine, self.accelerator.device
        n = len(queries)
        if not (n == len(responses) == len(scores)):
            raise ValueError(f"step: {n} queries, {len(responses)} responses, {len(scores)} scores")
        if n != cfg.batch_size:
            raise ValueError(f"step: batch size {n} does not match config.batch_size {cfg.batch_size}")
        ids, mask, labels = self._build_batch(queries, responses)
        scores_t = torch.tensor([float(x) for x in scores], dtype=torch.float32)
        mbs = cfg.mini_batch_size
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if self.time_phases else None
        if ev:
            ev[0].record()
        # ---- rollout: no-grad, eval mode, in chunks of mini_batch_size rows
        was_training = model.training
        model.eval()
        old_logp, old_values, ref_logp, lens = [], [], [], []
        try:
            with torch.no_grad():
                for lo in range(0, n, mbs):
                    rows = list(range(lo, min(lo + mbs, n)))
                    i_, m_, l_, g_ = ids[rows], mask[rows], labels[rows], self._rows_images(ids, img, rows)
                    lp, _, v = model(i_.to(dev), m_.to(dev), l_.to(dev), **g_)
                    so = model.seq_off.tolist()
                    lens += [so[j + 1] - so[j] for j in range(len(rows))]
                    old_logp.append(lp.clone())
                    old_values.append(v.clone())
                    ref_logp.append(self._reference_logps(i_, m_, l_, g_).clone())
        finally:
            model.train(was_training)
        old_logp, old_values, ref_logp = torch.cat(old_logp), torch.cat(old_values), torch.cat(ref_logp)
        seq_off = [0]
        for L in lens:
            seq_off.append(seq_off[-1] + L)
        R = seq_off[-1]
        if R < 2:
            raise ValueError(f"step: whitening needs at least 2 response tokens in the batch, got {R}")
        # ---- rewards, advantages, returns
        adv, ret = torch.empty(R, dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.float32, device=dev)
        kl_sums, astats = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(4, dtype=torch.float32, device=dev)
        _hip.call("vlr_ppo_advantages", old_logp, ref_logp, old_values, torch.tensor(seq_off, dtype=torch.int32, device=dev), scores_t.to(dev),
                  float(self.kl_ctl.value), KL_PENALTY_IDS[cfg.kl_penalty], float(cfg.gamma), float(cfg.lam), int(bool(cfg.whiten_rewards)),
                  adv, ret, kl_sums, astats, R, n)
        if ev:
            ev[1].record()
        # ---- optimisation (train mode for its passes; the caller's mode comes back afterwards)
        model.train()
        upstream = 1.0 / cfg.gradient_accumulation_steps
        mb_stats, mb_ent = [], []
        try:
            for _ in range(cfg.ppo_epochs):
                perm = torch.randperm(n, generator=self._perm_gen).tolist()
                for b0 in range(0, n, cfg.backward_batch_size):
                    eng.zero_grad()
                    for m0 in range(b0, b0 + cfg.backward_batch_size, mbs):
                        rows = perm[m0:m0 + mbs]
                        tok_idx = torch.tensor([t for r in rows for t in range(seq_off[r], seq_off[r + 1])], dtype=torch.long, device=dev)
                        Rm = tok_idx.numel()
                        if Rm < 2:
                            raise ValueError(f"step: a minibatch needs at least 2 response tokens, got {Rm}")
                        if cfg.log_entropy:
                            logp, _, vpred, ent = model(ids[rows].to(dev), mask[rows].to(dev), labels[rows].to(dev), return_entropy=True,
                                                        **self._rows_images(ids, img, rows))
                            mb_ent.append(ent.mean())
                        else:
                            logp, _, vpred = model(ids[rows].to(dev), mask[rows].to(dev), labels[rows].to(dev), **self._rows_images(ids, img, rows))
                        dlogp, dvpred = torch.empty_like(logp), torch.empty_like(vpred)
                        st = torch.empty(17, dtype=torch.float32, device=dev)
                        _hip.call("vlr_ppo_loss", logp.detach(), vpred.detach(), old_logp[tok_idx], old_values[tok_idx], adv[tok_idx], ret[tok_idx],
                                  Rm, float(cfg.cliprange), float(cfg.cliprange_value), float(cfg.vf_coef), float(cfg.ratio_threshold), upstream,
                                  dlogp, dvpred, st)
                        torch.autograd.backward([logp, vpred], [dlogp, dvpred])
                        mb_stats.append(st)
                    eng.optimizer_step(cfg.learning_rate, 0.9, 0.999, 1e-8, 0.0, cfg.max_grad_norm)
                # trl decides early stopping once per epoch, on the policykl of the epoch's last minibatch, after its optimizer steps
                # (_early_stop: policykl > 1.5 * target_kl -> zero_grad and no further epoch)
                if cfg.early_stopping and float(mb_stats[-1][4]) > 1.5 * cfg.target_kl:
                    eng.zero_grad()
                    break
        finally:
            model.train(was_training)
        if ev:
            ev[2].record()
            torch.cuda.synchronize()
            self.last_timing = dict(rollout_ms=ev[0].elapsed_time(ev[1]), optimisation_ms=ev[1].elapsed_time(ev[2]))
        # ---- stats (one device-to-host copy) and the KL controller
        ms = torch.stack(mb_stats).mean(0).tolist()
        a = astats.tolist()
        kl_coef = float(self.kl_ctl.value)
        qlen = [float(q.numel()) for q in queries]
        rlen = [float(r.numel()) for r in responses]
        stats = {
            "objective/kl": a[0], "objective/kl_coef": kl_coef,
            "ppo/loss/policy": ms[1], "ppo/loss/value": ms[2], "ppo/loss/total": ms[0],
            "ppo/policy/approxkl": ms[3], "ppo/policy/policykl": ms[4], "ppo/policy/clipfrac": ms[5], "ppo/policy/advantages_mean": ms[13],
            "ppo/policy/ratio": ms[7],
            "ppo/returns/mean": ms[8], "ppo/returns/var": ms[9],
            "ppo/val/vpred": ms[10], "ppo/val/error": ms[12], "ppo/val/clipfrac": ms[6], "ppo/val/mean": ms[14], "ppo/val/var": ms[15],
            "ppo/mean_scores": float(scores_t.mean()), "ppo/std_scores": float(scores_t.std()) if n > 1 else float("nan"),
            "ppo/mean_non_score_reward": a[1],
            "tokens/queries_len_mean": sum(qlen) / n, "tokens/responses_len_mean": sum(rlen) / n,
            "ppo/learning_rate": float(cfg.learning_rate),
        }
        if cfg.log_entropy:
            stats["ppo/policy/entropy"] = float(torch.stack(mb_ent).mean())
            stats["objective/entropy"] = sequence_neg_logp_mean(old_logp, seq_off)
        self.kl_ctl.update(a[0], cfg.batch_size)
        self.state.global_step += 1
        if self.keep_rollout:
            self.last_rollout = dict(old_logp=old_logp, old_values=old_values, ref_logp=ref_logp, seq_off=seq_off, advantages=adv, returns=ret,
                                     kl_sums=kl_sums, minibatch_stats=mb_stats)
        return stats


GRPO_LOSS_TYPES = {"grpo": 0, "bnpo": 1, "dr_grpo": 2}


@dataclasses.dataclass
class GRPOConfig:
    """Group Relative Policy Optimization: batch_size prompts (P) per step, num_generations samples (G) per prompt, P * G rows per
    step(); mini_batch_size rows per forward, mini_batch_size * gradient_accumulation_steps rows per optimizer step; num_iterations
    optimisation passes over one step's rows.  epsilon / epsilon_high bound the ratio at 1 - epsilon and 1 + epsilon_high (None:
    epsilon); beta weighs the per-token KL estimate against the reference (0: no reference pass at all).
    The policy entropy, from the lm-head pass the log-probs come from (all three off by default: the step is then launch for launch the
    one without them): log_entropy adds "grpo/entropy", the token-mean entropy of the training forward; top_entropy_quantile = q in
    (0, 1] restricts the policy term to the tokens of a minibatch whose entropy is at least the (1 - q) quantile of the minibatch's
    (trl's get_high_entropy_mask; 1: no mask) and adds "grpo/entropy_kept_frac"; entropy_coef subtracts entropy_coef * H_t from every
    token's loss."""
    learning_rate: float = 1e-6
    batch_size: int = 4
    num_generations: int = 8
    mini_batch_size: int = 8
    gradient_accumulation_steps: int = 1
    num_iterations: int = 1
    beta: float = 0.04
    epsilon: float = 0.2
    epsilon_high: Optional[float] = None
    loss_type: str = "grpo"
    scale_rewards: bool = True
    max_new_tokens: Optional[int] = None
    max_grad_norm: Optional[float] = None
    seed: int = 0
    world_size: int = 1
    use_lora: bool = False
    gradient_checkpointing: bool = False
    output_dir: Optional[str] = None
    per_device_gamelog_size: int = 2
    local_rank: int = -1
    save_steps: int = 0
    resume_from_checkpoint: Optional[str] = None
    log_entropy: bool = False
    top_entropy_quantile: float = 1.0
    entropy_coef: float = 0.0
    # generate(sampler="device") with seed = config.seed + 2 (see PPOConfig.device_sampler); off: the torch sampler on `_sample_gen`
    device_sampler: bool = False

    def __post_init__(self):
        if self.batch_size < 1:
            raise ValueError(f"batch_size ({self.batch_size}) must be at least 1 prompt")
        if not 0.0 < float(self.top_entropy_quantile) <= 1.0:
            raise ValueError(f"top_entropy_quantile ({self.top_entropy_quantile}) must lie in (0, 1]")
        if self.num_generations < 2:
            raise ValueError(f"num_generations ({self.num_generations}) must be at least 2: the advantage is the reward standardised inside "
                             "its group")
        self.rows = self.batch_size * self.num_generations
        self.backward_batch_size = self.mini_batch_size * self.gradient_accumulation_steps
        if self.mini_batch_size <= 0 or self.gradient_accumulation_steps <= 0 or self.rows % self.backward_batch_size:
            raise ValueError(f"batch_size * num_generations ({self.rows}) must be a multiple of mini_batch_size * gradient_accumulation_steps "
                             f"({self.backward_batch_size})")
        if self.num_iterations < 1:
            raise ValueError(f"num_iterations ({self.num_iterations}) must be at least 1")
        if self.beta < 0:
            raise ValueError(f"beta ({self.beta}) must not be negative")
        if self.epsilon < 0 or (self.epsilon_high is not None and self.epsilon_high < 0):
            raise ValueError(f"epsilon ({self.epsilon}) and epsilon_high ({self.epsilon_high}) must not be negative")
        if self.loss_type not in GRPO_LOSS_TYPES:
            raise ValueError(f"loss_type must be one of {sorted(GRPO_LOSS_TYPES)}, got {self.loss_type!r}")
        if self.loss_type == "dr_grpo" and (self.max_new_tokens is None or self.max_new_tokens < 1):
            raise ValueError("loss_type 'dr_grpo' divides by max_new_tokens: set it")
        if self.per_device_gamelog_size > self.rows:
            raise ValueError("per_device_gamelog_size should be less than batch_size * num_generations")


def high_entropy_mask(entropy, q):
    """trl's get_high_entropy_mask over one minibatch's R tokens: keep [R] uint8 = entropy >= torch.quantile(entropy, 1 - q) (linear
    interpolation; the entropy detached), on the tensor's device and without a host sync - a tie with the threshold is kept"""
    h = entropy.detach().float()
    return (h >= torch.quantile(h, 1.0 - float(q))).to(torch.uint8)


class VLGRPOTrainer(VLOnlineRLTrainer):
    """The GRPO step on the HIP engine (include/vlr.h "GRPO"): every prompt gets G samples from ONE call of the model's generate
    (num_return_sequences = G: one prefill per prompt, one decode batch), every sample one scalar reward, the advantage is the reward
    standardised inside its group (vlr_grpo_advantages), and the loss is the clipped per-token surrogate plus beta times a per-token KL
    estimate against the reference (vlr_grpo_loss).  The policy is a PLAIN family wrapper: no value head, no GAE, no whitening across
    the batch.  The no-grad passes are run only when their numbers are read: the old log-probs when a step's rows see more than one
    optimizer step (num_iterations > 1, or more rows than one backward batch) - otherwise the kernel takes NULL, the ratio is exactly 1
    and the gradient still flows - and the reference log-probs when beta != 0 (the adapters switched off under LoRA, else a frozen copy).

    Deliberate differences from trl's GRPOTrainer: the rows of a step are walked in generation order, never permuted; the image inputs
    are expanded per row, so the vision tower runs again on a repeated image; no-grad passes in eval mode; the entropy mask's quantile
    is taken per minibatch (top_entropy_quantile);
    scores come from a reward model (VLRewardModel.score) or from `reward_fn(queries_text, responses_text) -> list of floats`;
    world_size > 1 is refused: it has never been run."""

    def __init__(self, config=None, model=None, ref_model=None, reward_model=None, processor=None, dataset=None, data_collator=None,
                 generation_kwargs=None, reward_fn=None):
        if config is None or model is None:
            raise ValueError("VLGRPOTrainer needs a config and a model")
        if hasattr(model, "v_head"):
            raise ValueError("VLGRPOTrainer trains a plain family wrapper (LlavaForRL, QwenVLForRL): GRPO has no value head")
        if int(getattr(config, "world_size", 1) or 1) > 1 or _world() > 1:
            raise NotImplementedError("GRPO on more than one GPU has never been run on the MI355X path")
        if reward_model is not None and reward_fn is not None:
            raise ValueError("You can only use one of reward_model and reward_fn")
        self._init_shared(config, model, reward_model, processor, dataset, data_collator, generation_kwargs)
        self.reward_fn = reward_fn
        if ref_model is None and not self.is_peft_model and config.beta != 0:
            ref_model = model.create_reference_model()
            ref_model.eval()
        self.ref_model = ref_model
        self._sample_gen = torch.Generator(device=self.accelerator.device).manual_seed(int(config.seed) + 2)      # the sampler's own stream
        self.time_phases = False      # tools/grpo_bench.py: HIP events around the no-grad passes and the optimisation of step() -> last_timing
        self.keep_rollout = False     # True: step() leaves its tensors in last_rollout (diagnostics, the tests)
        self.last_rollout = None
        model.engine.init_optimizer()

    def _checkpoint_extra(self):
        return dict(sample_generator=self._sample_gen.get_state().tolist(), num_generations=self.config.num_generations,
                    **self._sampler_state())

    def _restore_extra(self, state, path):
        if int(state.get("num_generations", self.config.num_generations)) != self.config.num_generations:
            raise ValueError(f"resume_from_checkpoint: {path} was written with num_generations={state['num_generations']}, this run has "
                             f"{self.config.num_generations}")
        self._sample_gen.set_state(torch.tensor(state["sample_generator"], dtype=torch.uint8))
        self._restore_sampler_state(state)

    # ------------------------------------------------------------------------------------------ rows of a group
    def _expand_queries(self, queries):
        """the P queries as the P * G rows see them: row p * G + j carries query p"""
        G = self.config.num_generations
        return [queries[i // G] for i in range(len(queries) * G)]

    def _expand_images(self, queries, img):
        """the image inputs of P prompts -> those of the P * G rows, in repeat_interleave order (the rules of _rows_images)"""
        if not img:
            return {}
        G = self.config.num_generations
        T = max(int(q.numel()) for q in queries)
        ids = torch.full((len(queries), T), -1, dtype=torch.long)
        for p, q in enumerate(queries):
            ids[p, :q.numel()] = q.reshape(-1).cpu().long()
        return self._rows_images(ids, img, [p for p in range(len(queries)) for _ in range(G)])

    # ------------------------------------------------------------------------------------------ sampling
    @torch.no_grad()
    def generate(self, queries, generation_kwargs=None, **img):
        """ONE call of the model's own generate for all P queries: do_sample=True, num_return_sequences=G (one prefill per prompt, the
        samples decoded as one batch over the shared prompt cache where the model has it), the adapters live under LoRA
        (merge_lora=False).  -> P * G responses, row p * G + j being sample j of query p, each cut after its first stop."""
        kw = dict(self.generation_kwargs)
        kw.update(generation_kwargs or {})
        kw.update(do_sample=True, num_return_sequences=self.config.num_generations)
        if kw.get("generation_config") is not None:      # the model's generate reads do_sample from the generation config first: sample there too
            kw["generation_config"] = gc = copy.copy(kw["generation_config"])
            gc.do_sample, gc.num_return_sequences = True, self.config.num_generations
        kw.setdefault("generator", self._sample_gen)
        VLOnlineRLTrainer._device_sampler_kwargs(self, kw)
        if self.config.max_new_tokens is not None:
            kw.setdefault("max_new_tokens", int(self.config.max_new_tokens))
        if self.is_peft_model:
            kw.setdefault("merge_lora", False)
        queries = [q.reshape(-1).cpu().long() for q in queries]
        return self._generate_rows(queries, False, kw, img, fanout=self.config.num_generations)

    def _clipped_frac(self, responses):
        """fraction of the responses that ran to max_new_tokens without meeting a stop"""
        limit = self.config.max_new_tokens
        if limit is None:
            limit = getattr(self.generation_kwargs.get("generation_config"), "max_new_tokens", None)
        if limit is None:
            return 0.0
        eos, stops = self._stop_rules(self.model, self.generation_kwargs)
        cut = 0
        for r in responses:
            row = r.reshape(-1).tolist()
            stopped = row[-1] in eos or any(len(sq) <= len(row) and row[len(row) - len(sq):] == sq for sq in stops)
            cut += int(len(row) >= int(limit) and not stopped)
        return cut / len(responses)

    # ------------------------------------------------------------------------------------------ scoring
    def score(self, queries_text, responses_text, img):
        """one score per (query, response) row: the reward function when one was given, else the reward model (compute_scores)"""
        if self.reward_fn is not None:
            scores = [float(x) for x in self.reward_fn(queries_text, responses_text)]
            if len(scores) != len(responses_text):
                raise ValueError(f"reward_fn returned {len(scores)} scores for {len(responses_text)} responses")
            return scores
        if self.reward_model is None:
            raise NotImplementedError("GRPO needs a reward source: a reward_model (VLRewardModel) or a reward_fn")
        return [float(x) for x in self.compute_scores(queries_text, responses_text, img)]

    # ------------------------------------------------------------------------------------------ loop
    def train(self, resume_from_checkpoint=None):
        """per batch of P prompts: generate P * G responses, decode, score, step, log; a batch whose scoring raises is skipped;
        config.save_steps > 0 writes a checkpoint every so many steps, resume_from_checkpoint continues one"""
        if self.reward_fn is None and self.reward_model is None:
            raise NotImplementedError("GRPO needs a reward source: a reward_model (VLRewardModel) or a reward_fn")
        resume = resume_from_checkpoint or getattr(self.config, "resume_from_checkpoint", None)
        skip = 0
        if resume:
            skip = int(self.load_checkpoint(resume).get("batches_seen", 0))
        self.batches_seen = 0
        for batch in self.get_batches():
            self.batches_seen += 1
            if self.batches_seen <= skip:      # the rows a resumed run has already consumed (the row order is part of the checkpoint)
                continue
            queries = batch["input_ids"]
            img = {k: batch[k] for k in self.IMAGE_KEYS if k in batch}
            responses = self.generate(queries, **img)
            q_text = self._expand_queries(batch["query"])
            r_text = self.tokenizer.batch_decode(responses, skip_special_tokens=True)
            try:
                scores = self.score(q_text, r_text, self._expand_images(queries, img))
            except NotImplementedError:
                raise
            except Exception as e:      # as in PPO: warn, print the responses, skip the batch
                print(f"[grpo] WARNING: error when computing reward score, skipping this batch: {e!r}\n{r_text}", flush=True)
                self.skipped_batches = getattr(self, "skipped_batches", 0) + 1
                continue
            stats = self.step(queries, responses, scores, **img)
            k = self.config.per_device_gamelog_size
            game = [dict(query=self.processor.remove_image_placeholder(q), response=r, reward=float(s))
                    for q, r, s in zip(q_text[:k], r_text[:k], scores[:k])]
            self.log(dict(stats, game_log=game))
            if self.config.save_steps and self.state.global_step % self.config.save_steps == 0:
                self.save_checkpoint()
        return self.log_history

    # ------------------------------------------------------------------------------------------ step
    def _nograd_logps(self, which, ids, mask, labels, img):
        """token log-probs [R] of the policy ("old") or of the reference ("ref") on the response rows, under no-grad in eval mode"""
        from .model import token_logps
        dev = self.accelerator.device
        args = (ids.to(dev), mask.to(dev), labels.to(dev))
        if which == "old":
            return token_logps(self.model, *args, **img)
        if self.ref_model is None:
            with self.model.disable_adapter():
                return token_logps(self.model, *args, **img)
        return token_logps(self.ref_model, *args, **img)

    def step(self, queries, responses, scores, **img):
        """one GRPO step over P queries, their P * G responses (row p * G + j: sample j of query p) and P * G scores -> the stats dict.
        `img`: the image inputs of the P queries as the model's forward takes them; they are expanded per row and reach every pass."""
        from .model import token_logps
        cfg, model, eng, dev = self.config, self.model, self.model.engine, self.accelerator.device
        P, G, N = len(queries), cfg.num_generations, len(responses)
        if P != cfg.batch_size:
            raise ValueError(f"step: {P} queries do not match config.batch_size {cfg.batch_size}")
        if N != P * G or len(scores) != N:
            raise ValueError(f"step: {P} queries x num_generations {G} need {P * G} responses and scores, got {N} and {len(scores)}")
        ids, mask, labels = self._build_batch(self._expand_queries(queries), responses)
        img = self._expand_images(queries, img)
        mbs, bbs = cfg.mini_batch_size, cfg.backward_batch_size
        lens = [int(r.numel()) for r in responses]      # every response token is a labelled row (the first stop included)
        seq_off = [0]
        for L in lens:
            seq_off.append(seq_off[-1] + L)
        need_old = cfg.num_iterations > 1 or N > bbs
        need_ref = cfg.beta != 0
        q_ent, coef_ent = float(cfg.top_entropy_quantile), float(cfg.entropy_coef)
        use_ent = bool(cfg.log_entropy) or q_ent < 1.0 or coef_ent != 0.0      # any of the three: the lm-head pass with the entropy
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if self.time_phases else None
        if ev:
            ev[0].record()
        # ---- no-grad passes: eval mode, in chunks of mini_batch_size rows, only the ones whose numbers are read
        old_logp, ref_logp = None, None
        if need_old or need_ref:
            was_training = model.training
            model.eval()
            old, ref = [], []
            try:
                with torch.no_grad():
                    for lo in range(0, N, mbs):
                        rows = list(range(lo, min(lo + mbs, N)))
                        i_, m_, l_, g_ = ids[rows], mask[rows], labels[rows], self._rows_images(ids, img, rows)
                        if need_old:
                            old.append(self._nograd_logps("old", i_, m_, l_, g_).clone())
                        if need_ref:
                            ref.append(self._nograd_logps("ref", i_, m_, l_, g_).clone())
            finally:
                model.train(was_training)
            old_logp = torch.cat(old) if need_old else None
            ref_logp = torch.cat(ref) if need_ref else None
            for t in (old_logp, ref_logp):
                if t is not None and t.numel() != seq_off[-1]:
                    raise RuntimeError(f"step: {t.numel()} response rows for {seq_off[-1]} response tokens")
        # ---- advantages: the scores standardised inside their groups
        scores_t = torch.tensor([float(x) for x in scores], dtype=torch.float32, device=dev)
        adv, astats = torch.empty(N, dtype=torch.float32, device=dev), torch.empty(4, dtype=torch.float32, device=dev)
        _hip.call("vlr_grpo_advantages", scores_t, P, G, int(bool(cfg.scale_rewards)), adv, astats)
        if ev:
            ev[1].record()
        # ---- optimisation: num_iterations passes over the rows in generation order
        was_training = model.training
        model.train()
        upstream = 1.0 / cfg.gradient_accumulation_steps
        eps_high = cfg.epsilon if cfg.epsilon_high is None else cfg.epsilon_high
        mcl = int(cfg.max_new_tokens) if cfg.max_new_tokens is not None else 0
        mb_stats, mb_ent = [], []
        try:
            for _ in range(cfg.num_iterations):
                for b0 in range(0, N, bbs):
                    eng.zero_grad()
                    for m0 in range(b0, b0 + bbs, mbs):
                        rows = list(range(m0, m0 + mbs))
                        t0, t1 = seq_off[m0], seq_off[m0 + mbs]
                        so = torch.tensor([x - t0 for x in seq_off[m0:m0 + mbs + 1]], dtype=torch.int32, device=dev)
                        logp = token_logps(model, ids[rows].to(dev), mask[rows].to(dev), labels[rows].to(dev), return_entropy=use_ent,
                                           **self._rows_images(ids, img, rows))
                        ent = None
                        if use_ent:
                            logp, ent = logp
                        if logp.numel() != t1 - t0:
                            raise RuntimeError(f"step: {logp.numel()} response rows for {t1 - t0} response tokens")
                        dlogp = torch.empty_like(logp)
                        if not use_ent:
                            st = torch.empty(8, dtype=torch.float32, device=dev)
                            _hip.call("vlr_grpo_loss", logp.detach(), old_logp[t0:t1] if need_old else None, ref_logp[t0:t1] if need_ref else None,
                                      adv[m0:m0 + mbs], so, t1 - t0, mbs, float(cfg.epsilon), float(eps_high), float(cfg.beta),
                                      GRPO_LOSS_TYPES[cfg.loss_type], mcl, upstream, dlogp, st)
                            logp.backward(dlogp)
                        else:
                            keep = None
                            if q_ent < 1.0:      # trl's get_high_entropy_mask on the minibatch's tokens; stays on the device
                                keep = high_entropy_mask(ent, q_ent)
                            st = torch.empty(10, dtype=torch.float32, device=dev)
                            dent = torch.empty_like(logp)
                            _hip.call("vlr_grpo_loss_ent", logp.detach(), old_logp[t0:t1] if need_old else None,
                                      ref_logp[t0:t1] if need_ref else None, adv[m0:m0 + mbs], so, t1 - t0, mbs, float(cfg.epsilon), float(eps_high),
                                      float(cfg.beta), GRPO_LOSS_TYPES[cfg.loss_type], mcl, upstream, ent.detach(), keep, coef_ent, dlogp, dent, st)
                            if self.keep_rollout:
                                mb_ent.append((ent.detach(), keep))
                            if coef_ent != 0.0:      # the bonus reaches the weights through the lm-head backward with the entropy term
                                torch.autograd.backward([logp, ent], [dlogp, dent])
                            else:
                                logp.backward(dlogp)
                        mb_stats.append(st)
                    eng.optimizer_step(cfg.learning_rate, 0.9, 0.999, 1e-8, 0.0, cfg.max_grad_norm)
        finally:
            model.train(was_training)
        if ev:
            ev[2].record()
            torch.cuda.synchronize()
            self.last_timing = dict(nograd_ms=ev[0].elapsed_time(ev[1]), optimisation_ms=ev[1].elapsed_time(ev[2]))
        # ---- stats: one device-to-host copy
        flat = torch.cat([torch.stack(mb_stats).mean(0), astats]).tolist()
        ms, a = flat[:-4], flat[-4:]
        stats = {
            "grpo/loss": ms[0], "grpo/kl": ms[1], "grpo/ratio": ms[5],
            "grpo/clip_ratio/low": ms[2], "grpo/clip_ratio/high": ms[3], "grpo/clip_ratio/region": ms[4],
            "grpo/reward_mean": a[0], "grpo/reward_std": a[1], "grpo/frac_reward_zero_std": a[2],
            "grpo/clipped_completions_frac": self._clipped_frac(responses),
            "tokens/queries_len_mean": sum(float(q.numel()) for q in queries) / P, "tokens/responses_len_mean": sum(lens) / N,
            "grpo/learning_rate": float(cfg.learning_rate),
        }
        if cfg.log_entropy:
            stats["grpo/entropy"] = ms[8]
        if q_ent < 1.0:
            stats["grpo/entropy_kept_frac"] = ms[9]
        self.state.global_step += 1
        if self.keep_rollout:
            self.last_rollout = dict(old_logp=old_logp, ref_logp=ref_logp, seq_off=seq_off, advantages=adv, adv_stats=astats, minibatch_stats=mb_stats)
            if use_ent:      # per minibatch: (entropy [R], keep [R] uint8 or None)
                self.last_rollout["minibatch_entropy"] = mb_ent
        return stats


class _State:
    global_step = 0


class _Accelerator:
    """the two attributes of accelerate.Accelerator the reference trainer touches on this path."""

    def __init__(self, model):
        eng = getattr(model, "engine", None)
        self.device = eng.dev if eng is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")


def _world():
    import torch.distributed as dist
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _rank():
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def _backend():
    import torch.distributed as dist
    return dist.get_backend() if dist.is_available() and dist.is_initialized() else None
