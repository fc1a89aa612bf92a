"""Oracle side of the reward-model tests (checker only): rewards from the CPU oracles' final hidden states on EACH HALF ALONE - the two
forwards of trl RewardTrainer.compute_loss, each padded to its own width, reward = rm_head(hidden[:, -1, :]) - the pair loss, torch
autograd through it and the restated clip + AdamW loop."""
import math

import torch
import torch.nn.functional as F

from oracle import llava_dpo_oracle as O
from oracle import qwenvl_oracle as Q

HEAD_BIAS = 0.25


def rm_head(H, seed=7):
    """the head of the tests: w ~ U(-1, 1) / sqrt(H) from a seeded host generator, bias 0.25 -> (w [H] fp32, b [1] fp32)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(H, generator=g) * 2 - 1) / math.sqrt(H), torch.tensor([HEAD_BIAS])


def rm_batch(batch):
    """a DPO fixture batch as the RM collator would hand it over: ids and masks of both sides, each at its own width"""
    return dict(input_ids_chosen=batch["chosen_input_ids"], attention_mask_chosen=batch["chosen_attention_mask"],
                input_ids_rejected=batch["rejected_input_ids"], attention_mask_rejected=batch["rejected_attention_mask"],
                img_input_dict=dict(batch["img_input_dict"]), img_path=list(batch.get("img_path", [])))


def half_hidden(W, cfg, ids, mask, px, emulate=False):
    """final (post-norm) hidden states [B, S, H] of ONE half through the family's oracle forward"""
    if cfg.get("family") == "qwen_vl" or "visual" in cfg:
        return Q.qwenvl_forward(W, cfg, ids, mask, px.float(), emulate_bf16=emulate, return_hidden=True, dedupe_images=False)[0]
    return O.llava_forward(W, cfg, ids, mask, None, px.float(), emulate_bf16=emulate, dedupe_images=False, return_hidden=True)[0]


def rewards(W, cfg, rb, w, b, emulate=False):
    """(r_chosen [B], r_rejected [B]): rm_head at the LAST column of each half's own padded batch"""
    px = rb["img_input_dict"]["pixel_values"]
    out = []
    for side in ("chosen", "rejected"):
        h = half_hidden(W, cfg, rb[f"input_ids_{side}"], rb[f"attention_mask_{side}"], px, emulate)
        out.append(h[:, -1, :].float() @ w.float() + b.float())
    return out[0], out[1]


def pair_loss(rc, rr):
    return -F.logsigmoid(rc - rr).mean()


def accuracy(rc, rr):
    """trl compute_accuracy: argmax over [r_chosen, r_rejected] == 0; numpy's argmax takes the first of a tie"""
    return float((rc >= rr).float().mean())


def loss_and_grads(W, cfg, rb, w, b, names, emulate=False):
    """-> (loss, rc, rr, {name: grad} incl. 'rm_head.weight' / 'rm_head.bias') by torch autograd through the oracle"""
    leaves = {k: W[k].clone().requires_grad_(True) for k in names}
    wl, bl = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    Wl = dict(W)
    Wl.update(leaves)
    rc, rr = rewards(Wl, cfg, rb, wl, bl, emulate)
    loss = pair_loss(rc, rr)
    loss.backward()
    g = {k: v.grad for k, v in leaves.items()}
    g["rm_head.weight"], g["rm_head.bias"] = wl.grad, bl.grad
    return loss.detach(), rc.detach(), rr.detach(), g


def train_loop(W, cfg, rb, w, b, optim, steps, emulate=False):
    """`steps` full fine-tune steps the way the HIP path stores things: fp32 master weights (head included), forward / backward on their
    bf16 rounding, restated clip + AdamW; the head's weight decays, its bias and the norms do not.  -> per-step losses"""
    names = O.trainable_names(W)
    master = {k: v.clone() for k, v in W.items()}
    master["rm_head.weight"], master["rm_head.bias"] = w.clone(), b.clone()
    state, losses = {}, []
    for _ in range(steps):
        Wp = {k: v.bfloat16().float() for k, v in master.items()}
        loss, _, _, g = loss_and_grads(Wp, cfg, rb, Wp["rm_head.weight"], Wp["rm_head.bias"], names, emulate)
        grads = {k: v for k, v in g.items() if v is not None}
        O.clip_grad_norm_(grads, optim["max_grad_norm"])
        with torch.no_grad():
            O.adamw_step(master, grads, state, optim["lr"], optim["beta1"], optim["beta2"], optim["eps"], optim["weight_decay"])
        losses.append(float(loss))
    return losses
