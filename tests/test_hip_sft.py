"""Supervised fine-tuning on the MI355X: the batch-mean cross-entropy kernel, the model wrappers' `loss`, one SFT step's gradients
(single- and multi-block lm-head backward), rows with eos holes in the key mask, bit-reproducibility, a short training run against
the oracle trajectory, the DPO path left untouched, the other three model families and `vlrlhf.sft.main` end to end.
The CPU oracle and the committed fp32 golden logits are checkers only.  Needs a real MI355X:  pytest -m gpu"""
import copy
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import llava_dpo_oracle as O  # noqa: E402  (checker only)
from tests.golden_util import TINY_CKPT_CFG, TINY_PROCESSOR, load_case, t, write_tiny_checkpoint  # noqa: E402
from tests.test_hip_e2e import EMU, PEFT, build, cosine, gpu, make_trainer, relmax  # noqa: E402,F401

TOL_CE = 2e-2          # the bound test_forward_matches_golden puts on the per-sequence AVERAGE log-prob of this fixture: the batch mean is a
#                        count-weighted mean of those averages, so it cannot be further off


def ref_ce(logits, labels, mask=None):
    """the reference wrappers' loss lines in plain torch: CrossEntropyLoss over the shifted positions (that the shifted mask keeps)"""
    sl, lab = logits[:, :-1], labels[:, 1:]
    if mask is not None:
        keep = mask[:, 1:] != 0
        return F.cross_entropy(sl[keep].double(), lab[keep])
    return F.cross_entropy(sl.reshape(-1, sl.shape[-1]).double(), lab.reshape(-1))


def sft_inputs(cfg, batch, dev):
    """the fixture's concatenated (chosen ; rejected) batch as an SFT batch: what the golden logits / merged labels were made from"""
    from vlrlhf.models.Llava import LlavaDPOTrainer
    tr = LlavaDPOTrainer.__new__(LlavaDPOTrainer)
    tr.is_encoder_decoder, tr.label_pad_token_id, tr.padding_value = False, -100, 0
    tr.accelerator = SimpleNamespace(device=dev)
    cb = tr.concatenated_inputs(batch, device=dev)
    return dict(input_ids=cb["concatenated_input_ids"], attention_mask=cb["concatenated_attention_mask"], labels=cb["concatenated_labels"],
                **cb["concatenated_img_input_dict"])


def sft_trainer(model, cfg, cls=None, **kw):
    from vlrlhf.models.Llava import LlavaSFTTRainer
    o = cfg.get("optim", dict(lr=1e-3, beta1=0.9, beta2=0.98, eps=1e-6, weight_decay=0.05, max_grad_norm=1.0))
    args = SimpleNamespace(gradient_accumulation_steps=1, per_device_train_batch_size=2, learning_rate=o["lr"], adam_beta1=o["beta1"],
                           adam_beta2=o["beta2"], adam_epsilon=o["eps"], weight_decay=o["weight_decay"], max_grad_norm=o["max_grad_norm"], seed=0)
    return (cls or LlavaSFTTRainer)(model=model, args=args, **kw)


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("R", [1, 255, 256, 4097, 65536])
def test_ce_mean_kernel_matches_fp64_and_is_bit_reproducible(gpu, R):
    """fp32 summation of <= 65 536 terms with fp32 partials: relative error <= 1e-6 against fp64; two calls bit-equal"""
    from vlrlhf import _hip
    g = torch.Generator().manual_seed(R)
    tok = (-8.0 * torch.rand(R, generator=g) - 1e-3).cuda()
    ws = torch.empty(_hip.helper("vlr_ce_mean_workspace_bytes"), dtype=torch.uint8, device="cuda")
    outs = []
    for _ in range(2):
        out3 = torch.full((3,), float("nan"), device="cuda")
        _hip.call("vlr_ce_mean_fwd", tok, R, ws, out3)
        torch.cuda.synchronize()
        outs.append(out3.cpu())
    exp = float(-tok.double().sum() / R)
    rel = abs(float(outs[0][0]) - exp) / abs(exp)
    print(f"[ce_mean] R={R} loss={float(outs[0][0]):.8f} fp64={exp:.8f} rel={rel:.2e}")
    assert rel <= 1e-6, (R, rel)
    assert float(outs[0][1]) == float(R) and float(outs[0][2]) == pytest.approx(-1.0 / R, rel=1e-7)
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------------------ 2
def test_model_loss_matches_ce_of_golden_logits(gpu):
    z, cfg, W, W_ref, batch, rows = load_case("llava_hipsmall")
    model, _ = build(cfg, W, W_ref)
    inp = sft_inputs(cfg, batch, gpu)
    exp = float(ref_ce(t(z, "logits"), t(z, "merged_labels"), t(z, "merged_mask")))
    model.eval()
    with torch.no_grad():
        out = model(**inp)
        assert out.__dict__["loss"] is None, "the loss is computed when it is read, not by forward"
        loss = out.loss
    assert out["loss"] is loss and model.causal_lm_loss(out) is loss              # computed once
    print(f"[sft loss] hip={float(loss):.6f} golden fp32 CE={exp:.6f} |diff|={abs(float(loss) - exp):.2e}")
    assert abs(float(loss) - exp) < TOL_CE
    with torch.no_grad():
        assert model(**{k: v for k, v in inp.items() if k != "labels"}).loss is None          # no labels, no loss (reference :245)


# ------------------------------------------------------------------------------------------------------------ 3
def _sft_step(cfg, W, W_ref, inp, row_block=None, lora=None, ckpt=False):
    model, _ = build(cfg, W, W_ref)
    tr = sft_trainer(model, cfg, **(dict(peft_config=lora) if lora else {}))
    model.engine.ce_row_block = row_block
    if ckpt:
        model.gradient_checkpointing_enable()
    model.engine.init_optimizer()
    loss = tr.training_step(model, inp)
    torch.cuda.synchronize()
    return model, tr, loss


def test_sft_step_gradients_match_oracle_autograd_single_and_multi_block(gpu):
    """one SFT step against torch autograd through the CPU oracle's forward (fp32, the fixture's weights): per-tensor cosine > 0.995 and
    relative max < 8e-2 (the bounds of test_train_step_matches_golden), no tensor skipped - with the lm-head backward in ONE block and
    in blocks of 8 rows.  d hidden - and through it every gradient but lm_head's - depends on a row's own operands only: bit-identical
    across block sizes.  d W_lm sums over the rows; each block's product is rounded to bf16 as it is added to the gradient buffer, so
    bit-identity with the single-block sum cannot hold for it (include/vlr.h): it meets the same bounds instead."""
    z, cfg, W, W_ref, batch, rows = load_case("llava_hipsmall")
    inp = sft_inputs(cfg, batch, gpu)
    names = O.trainable_names(W)
    leaves = {k: W[k].clone().requires_grad_(True) for k in names}
    Wl = dict(W)
    Wl.update(leaves)
    cpu = {k: v.cpu() for k, v in inp.items()}
    logits, mlabels, aux = O.llava_forward(Wl, cfg, cpu["input_ids"], cpu["attention_mask"], cpu["labels"], cpu["pixel_values"].float())
    exp_loss = ref_ce(logits, mlabels, aux["mask"])
    exp_loss.backward()
    runs = {}
    for rb in (None, 8):
        model, tr, loss = _sft_step(cfg, W, W_ref, inp, row_block=rb)
        assert abs(float(loss) - float(exp_loss.detach())) < TOL_CE, (rb, float(loss), float(exp_loss.detach()))
        named = dict(model.named_parameters())
        assert set(named) == set(names), set(named) ^ set(names)
        for name in names:
            cs, rm = cosine(named[name].grad, leaves[name].grad), relmax(named[name].grad, leaves[name].grad)
            print(f"[sft grads] row_block={rb} {name}: cosine {cs:.5f} relmax {rm:.3e}")
            assert cs > 0.995 and rm < 8e-2, (rb, name, cs, rm)
        runs[rb] = (float(loss), {k: v.grad.clone() for k, v in named.items()})
    R = int((t(z, "merged_labels")[:, 1:].ne(-100) & t(z, "merged_mask")[:, 1:].ne(0)).sum())
    assert R > 3 * 8, "several blocks must have run"
    assert runs[None][0] == runs[8][0]
    for name in names:
        if name == "language_model.lm_head.weight":
            continue                                  # block-order bf16 accumulation: within the bounds above, not bit-equal
        assert torch.equal(runs[None][1][name], runs[8][1][name]), name


# ------------------------------------------------------------------------------------------------------------ 4
def _tiny_sft_setup(n_rows=8, max_seq_length=64):
    from vlrlhf.models.Llava import LlavaForRL, LlavaProcessor, LlavaSFTDataCollatorWithPadding, LlavaSFTTRainer
    from vlrlhf.utils.data import DATASET_MAP
    cfg = dict(TINY_CKPT_CFG)
    W = {k: v.bfloat16().float() for k, v in O.random_weights(cfg, seed=5, std=0.05).items()}
    proc = LlavaProcessor(TINY_PROCESSOR)
    proc.train()
    rows = DATASET_MAP["synthetic_conversations"](SimpleNamespace(synthetic_rows=n_rows, synthetic_image_size=cfg["image_size"]))
    model = LlavaForRL.from_state_dict(cfg, W)
    col = LlavaSFTDataCollatorWithPadding(proc.tokenizer.pad_token_id, -100, proc)
    tr = sft_trainer(model, cfg, LlavaSFTTRainer, processor=proc, train_dataset=rows, data_collator=col, max_seq_length=max_seq_length)
    return cfg, W, proc, model, tr, col


def _oracle_ce(W, cfg, b, emulate=False):
    logits, mlabels, aux = O.llava_forward(W, cfg, b["input_ids"], b["attention_mask"], b["labels"], b["pixel_values"].float(),
                                           emulate_bf16=emulate, dedupe_images=False)
    return ref_ce(logits, mlabels, aux["mask"])


def test_rows_with_eos_holes_in_the_key_mask(gpu):
    """rows built by tokenize_row: the eos tokens inside the conversation are masked keys with label -100.  They give no gradient (the
    eos embedding row's gradient is exactly zero - its only other occurrence, the appended last token, predicts nothing), the loss does
    not depend on WHICH token sits in a hole, and it equals the oracle's on the same ids, mask and labels."""
    cfg, W, proc, model, tr, col = _tiny_sft_setup()
    b = col(tr.train_dataset[:2])
    eos = proc.tokenizer.eos_token_id
    holes = (b["input_ids"] == eos) & (b["attention_mask"] == 0) & (b["labels"] == -100)
    assert int(holes.sum()) >= 2 and bool((b["attention_mask"][:, :-1].sum(1) < b["attention_mask"].shape[1] - 1).all())
    exp = float(_oracle_ce(W, cfg, b))
    loss = tr.training_step(model, b)
    torch.cuda.synchronize()
    print(f"[sft holes] hip={float(loss):.6f} oracle={exp:.6f}")
    assert abs(float(loss) - exp) < TOL_CE
    emb = dict(model.named_parameters())["language_model.model.embed_tokens.weight"].grad.float()
    assert float(emb[eos].abs().sum()) == 0.0 and float(emb.abs().sum()) > 0
    b2 = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}
    b2["input_ids"][holes] = 5                       # another token in the holes: masked out of attention, label -100 -> the same bits
    model.engine.zero_grad()
    loss2 = tr.training_step(model, b2)
    assert float(loss2) == float(loss)


# ------------------------------------------------------------------------------------------------------------ 5
def test_sft_step_is_bit_reproducible_checkpointing_identical_and_lora_trains_adapters_only(gpu):
    z, cfg, W, W_ref, batch, rows = load_case("llava_hipsmall")
    inp = sft_inputs(cfg, batch, gpu)
    o = cfg["optim"]
    outs = []
    for ckpt in (False, False, True):
        model, tr, loss = _sft_step(cfg, W, W_ref, inp, ckpt=ckpt)
        g = model.engine.grads.clone()
        model.engine.optimizer_step(o["lr"], o["beta1"], o["beta2"], o["eps"], o["weight_decay"], o["max_grad_norm"])
        model.engine.wait_optimizer()
        torch.cuda.synchronize()
        outs.append((float(loss), g, model.engine.policy.flat.clone()))
    for other in outs[1:]:             # the same step twice; gradient checkpointing on
        assert outs[0][0] == other[0] and torch.equal(outs[0][1], other[1]) and torch.equal(outs[0][2], other[2])
    assert float(outs[0][1].float().abs().sum()) > 0
    model, tr, loss = _sft_step(cfg, W, W_ref, inp, lora=dict(PEFT, seed=5))
    eng = model.engine
    base, ad = eng.policy.flat.clone(), eng.lora_flat.clone()
    assert tr.is_peft_model and float(eng.lora_grads.float().abs().sum()) > 0
    eng.optimizer_step(o["lr"], o["beta1"], o["beta2"], o["eps"], o["weight_decay"], o["max_grad_norm"])
    eng.wait_optimizer()
    torch.cuda.synchronize()
    assert torch.equal(base, eng.policy.flat) and not torch.equal(ad, eng.lora_flat)


# ------------------------------------------------------------------------------------------------------------ 6
def test_sft_run_loss_falls_and_tracks_oracle_trajectory(gpu):
    """20 optimizer steps over four batches of the synthetic multi-turn conversations, lr 2e-4 (the rate of
    test_training_trajectory_tracks_oracle): the loss falls, and every step is within that test's 3e-2 of the oracle trajectory computed the
    way the HIP path stores things (fp32 master weights, restated clip + AdamW, forward / backward on their bf16 rounding)."""
    cfg, W, proc, model, tr, col = _tiny_sft_setup()
    o = dict(lr=2e-4, beta1=0.9, beta2=0.98, eps=1e-6, weight_decay=0.05, max_grad_norm=1.0)
    batches = [col(tr.train_dataset[i:i + 2]) for i in range(0, 8, 2)]
    eng = model.engine
    eng.init_optimizer()
    hip = []
    for s in range(20):
        eng.zero_grad()
        hip.append(float(tr.training_step(model, batches[s % 4])))
        eng.optimizer_step(o["lr"], o["beta1"], o["beta2"], o["eps"], o["weight_decay"], o["max_grad_norm"])
    torch.cuda.synchronize()
    names = O.trainable_names(W)
    master = {k: v.clone() for k, v in W.items()}
    state, ora = {}, []
    for s in range(20):
        leaves = {k: master[k].bfloat16().float().requires_grad_(True) for k in names}
        Wp = {k: v.bfloat16().float() for k, v in master.items()}
        Wp.update(leaves)
        loss = _oracle_ce(Wp, cfg, batches[s % 4], emulate=EMU).float()
        loss.backward()
        grads = {k: leaves[k].grad for k in names if leaves[k].grad is not None}
        O.clip_grad_norm_(grads, o["max_grad_norm"])
        with torch.no_grad():
            O.adamw_step(master, grads, state, o["lr"], o["beta1"], o["beta2"], o["eps"], o["weight_decay"])
        ora.append(float(loss))
    print("[sft run] hip   ", " ".join(f"{x:.4f}" for x in hip))
    print("[sft run] oracle", " ".join(f"{x:.4f}" for x in ora))
    print("[sft run] worst |diff|", max(abs(h - r) for h, r in zip(hip, ora)))
    assert sum(hip[-4:]) < sum(hip[:4]) and sum(ora[-4:]) < sum(ora[:4]), (hip, ora)
    for h, r in zip(hip, ora):
        assert abs(h - r) < 3e-2, (hip, ora)


# ------------------------------------------------------------------------------------------------------------ 7
def test_dpo_step_is_bit_identical_before_and_after_the_sft_path(gpu):
    z, cfg, W, W_ref, batch, rows = load_case("llava_hipsmall")

    def dpo_step():
        model, ref = build(cfg, W, W_ref)
        tr = make_trainer(model, ref, cfg)
        loss = tr.training_step(model, batch)
        torch.cuda.synchronize()
        return float(loss), model.engine.grads.clone()
    before = dpo_step()
    _sft_step(cfg, W, W_ref, sft_inputs(cfg, batch, gpu), row_block=8)
    # and on ONE model: an SFT loss read between two DPO steps leaves the second exactly where a fresh model puts it
    model, ref = build(cfg, W, W_ref)
    tr = make_trainer(model, ref, cfg)
    with torch.no_grad():
        assert torch.isfinite(model(**sft_inputs(cfg, batch, gpu)).loss)
    loss = tr.training_step(model, batch)
    torch.cuda.synchronize()
    after = dpo_step()
    assert before[0] == after[0] == float(loss)
    assert torch.equal(before[1], after[1]) and torch.equal(before[1], model.engine.grads)


# ------------------------------------------------------------------------------------------------------------ 8
def _family(name):
    if name == "llavanext":
        from tests.test_hip_llavanext import build as b
        z, cfg, W, W_ref, batch, model, ref, mk = b()
        return z, model, mk("sigmoid"), batch, t(z, "merged_labels"), t(z, "merged_mask")
    if name == "qwenvl":
        from tests.test_hip_qwenvl import build as b
        z, cfg, W, W_ref, batch, model, ref, tr = b()
        return z, model, tr, batch, None, None
    from tests.test_hip_internlm import build as b
    z, cfg, W, W_ref, batch, model, ref, tr = b()
    return z, model, tr, batch, t(z, "merged_labels"), None


@pytest.mark.parametrize("family", ["llavanext", "qwenvl", "internlm"])
def test_other_families_forward_loss_backward(gpu, family):
    """forward(labels) -> .loss -> backward on each family's committed toy fixture, against the cross-entropy of the fixture's fp32 golden
    logits (made by the reference's own classes through oracle/make_golden_*.py) under that family's row rule: LLaVA-Next selects by the
    shifted merged mask, Qwen-VL and InternLM-XComposer2 by the label alone."""
    z, model, tr, batch, labels, mask = _family(family)
    cb = tr.concatenated_inputs(batch, device=torch.device("cuda"))
    inp = dict(input_ids=cb["concatenated_input_ids"], attention_mask=cb["concatenated_attention_mask"], labels=cb["concatenated_labels"],
               **cb["concatenated_img_input_dict"])
    labels = labels if labels is not None else cb["concatenated_labels"].cpu()
    exp = float(ref_ce(t(z, "logits"), labels, mask))
    model.train()
    out = model(**inp)
    loss = out.loss
    print(f"[sft {family}] hip={float(loss):.6f} golden fp32 CE={exp:.6f} |diff|={abs(float(loss) - exp):.2e}")
    assert abs(float(loss) - exp) < TOL_CE
    loss.backward()
    torch.cuda.synchronize()
    g = model.engine.grads.float()
    assert bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0


# ------------------------------------------------------------------------------------------------------------ 9
def _args(ckpt, out, **kw):
    a = dict(model_name_or_path=ckpt, dataset_name="synthetic_conversations", synthetic_rows=26, synthetic_image_size=28, output_dir=out,
             per_device_train_batch_size=2, max_steps=4, logging_steps=2, learning_rate=1e-4, max_length=64, warmup_ratio=0.0,
             lr_scheduler_type="constant", dataloader_prefetch=2, seed=3)
    a.update(kw)
    return [x for k, v in a.items() for x in (f"--{k}", str(v))]


def test_sft_main_end_to_end(tmp_path):
    from safetensors.torch import load_file
    from vlrlhf import sft
    from vlrlhf.models.Llava import LlavaForRL
    ckpt = str(tmp_path / "ckpt")
    write_tiny_checkpoint(ckpt)
    out = str(tmp_path / "full")
    tr = sft.main(_args(ckpt, out, save_strategy="steps", save_steps=2, save_total_limit=2, eval_strategy="steps", eval_steps=2,
                        gradient_accumulation_steps=2))
    hist = [h for h in tr.log_history if "loss" in h]
    assert len(hist) == 2 and hist[-1]["step"] == 4 and {"loss", "learning_rate", "grad_norm", "epoch"} <= set(hist[-1])
    assert all(torch.isfinite(torch.tensor(h["loss"])) for h in hist)
    assert any("eval_loss" in h for h in tr.log_history)
    for fn in ("checkpoint-4/trainer_state.json", "checkpoint-4/model.safetensors", "checkpoint-4/optimizer_master.safetensors",
               "config.json", "model.safetensors", "tokenizer.json", "trainer_state.json"):
        assert os.path.isfile(os.path.join(out, fn)), fn
    tr.model.engine.wait_optimizer()
    torch.cuda.synchronize()
    assert torch.equal(LlavaForRL.from_pretrained(out).engine.policy.flat, tr.model.engine.policy.flat)
    assert not torch.equal(LlavaForRL.from_pretrained(ckpt).engine.policy.flat, tr.model.engine.policy.flat)
    del tr
    out = str(tmp_path / "lora")
    tr = sft.main(_args(ckpt, out, use_lora="true", lora_r=8, lora_alpha=16, lora_dropout=0.0, max_steps=2, logging_steps=1,
                        merge_peft_model="true"))
    sd = load_file(os.path.join(out, "adapter_model.safetensors"))
    assert os.path.isfile(os.path.join(out, "adapter_config.json")) and all(".lora_A.weight" in k or ".lora_B.weight" in k for k in sd)
    assert any(float(v.float().abs().sum()) > 0 for k, v in sd.items() if ".lora_B.weight" in k), "the adapters did not train"
    assert os.path.isfile(os.path.join(out, "merged", "config.json")) and os.path.isfile(os.path.join(out, "merged", "model.safetensors"))
    merged, base = LlavaForRL.from_pretrained(os.path.join(out, "merged")), LlavaForRL.from_pretrained(ckpt)
    assert not torch.equal(merged.engine.policy.flat, base.engine.policy.flat)
