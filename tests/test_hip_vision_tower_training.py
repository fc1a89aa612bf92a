"""Training the CLIP vision tower (cfg["train_vision_tower"], --freeze_vision_tower False) end to end on the LLaVA-1.5 and LLaVA-Next
fixtures: the step with the tower trainable against the frozen step of the same build (bit-identical loss and decoder / projector
gradients - the forward is the same code), every tower gradient against fp32 autograd through the CPU oracle, the tensors the forward
never evaluates, a two-step clip + AdamW trajectory, the reference pass (the initial tower: it does not move), save / resume, and
one SFT step.

Gradient bounds: the project's (test_train_step_matches_golden: cosine > 0.995, relative max < 8e-2).  Where a tower tensor needs
more, its bound is 2 x the distance between the fp32 oracle gradient and the oracle gradient computed with the rounding the HIP
path applies (O.HIP_ROUNDING) - computed here on the CPU and printed; the factor 2 because the kernels also round stored
intermediates the emulation keeps in fp32.  Measured on an MI355X, both fixtures and the SFT step: cosine >= 0.9996, relative max
<= 4.2e-2 on every tower tensor with a nonzero gradient (the oracles themselves: <= 3.2e-2 apart).  Needs a real MI355X:  pytest -m gpu"""
import math
import os
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import llava_dpo_oracle as O  # noqa: E402  (checker only)
from tests.golden_util import load_case  # noqa: E402
from tests.test_hip_e2e import EMU, cosine, gpu, relmax  # noqa: E402,F401

CASES = ("llava_hipsmall", "llavanext_small")
OPT = dict(lr=1e-3, beta1=0.9, beta2=0.98, eps=1e-6, weight_decay=0.05, max_grad_norm=1.0)
VT = "vision_tower."


def build(case, train, out_dir=None):
    z, cfg, W, W_ref, batch, rows = load_case(case)
    if case == "llava_hipsmall":
        from vlrlhf.models.Llava import LlavaDPOTrainer as Trainer, LlavaForRL as Model
    else:
        from vlrlhf.models.LlavaNext import LlavaNextDPOTrainer as Trainer, LlavaNextForRL as Model
    model = Model.from_state_dict(dict(cfg, train_vision_tower=True) if train else cfg, W)
    ref = model.create_reference_model()
    ref.weights.load_state_dict(W_ref)
    args = SimpleNamespace(gradient_accumulation_steps=1, per_device_train_batch_size=2, learning_rate=OPT["lr"], adam_beta1=OPT["beta1"],
                           adam_beta2=OPT["beta2"], adam_epsilon=OPT["eps"], weight_decay=OPT["weight_decay"], max_grad_norm=OPT["max_grad_norm"],
                           seed=0, output_dir=str(out_dir) if out_dir is not None else "output")
    tr = Trainer(model, ref, cfg["beta"], 0, "sigmoid", args, None, -100, 0)
    return SimpleNamespace(z=z, cfg=cfg, W=W, W_ref=W_ref, batch=batch, model=model, ref=ref, tr=tr, eng=model.engine)


def step(b, optimize=True):
    b.eng.zero_grad()
    loss = b.tr.training_step(b.model, b.batch)
    out = b.eng.optimizer_step(OPT["lr"], OPT["beta1"], OPT["beta2"], OPT["eps"], OPT["weight_decay"], OPT["max_grad_norm"]) if optimize else None
    torch.cuda.synchronize()
    return loss, out


def bf(W):
    return {k: v.bfloat16().float() for k, v in W.items()}


_oracle = {}


def oracle_grads(case):
    """{name: gradient} of the DPO loss with every tensor of the model a leaf, through the fp32 oracle and through the oracle with the
    HIP path's rounding, on the bf16 weights the engine holds; computed once per fixture"""
    if case not in _oracle:
        z, cfg, W, W_ref, batch, rows = load_case(case)
        out = []
        for emu in (False, EMU):
            leaves = {k: v.clone().requires_grad_(True) for k, v in bf(W).items() if k in O.trainable_names(W, freeze_vision_tower=False)}
            loss, _ = O.compute_loss(leaves, bf(W_ref), cfg, batch, cfg["beta"], emulate_bf16=emu)
            loss.backward()
            out.append((float(loss), {k: v.grad for k, v in leaves.items()}))
        _oracle[case] = out
    return _oracle[case]


def unevaluated(W):
    last = max(int(k.split("encoder.layers.")[1].split(".")[0]) for k in W if "encoder.layers." in k)
    return {k for k in W if k.startswith(VT) and (f"encoder.layers.{last}." in k or "post_layernorm" in k)}


def check_grads(named, g32, gemu, names, what):
    for name in names:
        g, e = named[name].grad, g32[name]
        cs, rm = cosine(g, e), relmax(g, e)
        d_cs, d_rm = 1.0 - cosine(gemu[name], e), relmax(gemu[name], e)
        print(f"[{what}] {name}: cosine {cs:.5f} relmax {rm:.3e}; fp32 oracle <-> rounding oracle: 1-cosine {d_cs:.2e} relmax {d_rm:.3e}")
        if d_rm > 1.0:
            # The two oracles differ by more than the fp32 gradient's own size: that gradient is summation noise around an EXACT zero
            # (k_proj.bias: a bias on every key shifts all scores of a query equally, softmax does not see it), so a cosine or a
            # ratio to its largest element compares noise with noise (measured: the oracles 1.2e4 - 1.7e4 apart in relmax, the kernels
            # 2.8e4 - 4.8e4 from the fp32 one; 1 - cosine 0.8 - 1.25).  What can be asked of a gradient whose exact value is 0 is that it
            # is small on the scale of its sibling: d q_proj.bias is the same fixed-order column sum over the same rows of the same
            # d q|k|v buffer, so the project's relative-max bound is applied with the sibling's largest element as the denominator.
            sib = g32[name.replace("k_proj", "q_proj")]
            assert name.endswith("k_proj.bias") and float(e.abs().max()) < 1e-5 * float(sib.abs().max()), name
            zero = float(g.float().abs().max()) / float(sib.abs().max())
            print(f"[{what}] {name}: exact gradient 0; largest |g| = {zero:.3e} of the largest |d q_proj.bias|")
            assert zero < 8e-2, (name, zero)
            continue
        assert cs > min(0.995, 1.0 - 2.0 * d_cs) and rm < max(8e-2, 2.0 * d_rm), (name, cs, rm, d_cs, d_rm)


@pytest.mark.parametrize("case", CASES)
def test_first_step_parity_tower_gradients_and_unevaluated_tensors(gpu, case):
    fz, tn = build(case, False), build(case, True)
    loss_f, _ = step(fz, optimize=False)
    loss_t, _ = step(tn, optimize=False)
    # ---- the same forward, the same decoder / projector backward: bits
    assert float(loss_f) == float(loss_t)
    nf, nt = dict(fz.model.named_parameters()), dict(tn.model.named_parameters())
    assert set(nf) == set(O.trainable_names(tn.W)) and set(nt) - set(nf) == set(O.trainable_names(tn.W, False)) - set(nf) - unevaluated(tn.W)
    for name, p in nf.items():
        assert torch.equal(p.grad.view(torch.int16), nt[name].grad.view(torch.int16)), name
    # ---- every tower gradient against oracle autograd
    (l32, g32), (_, gemu) = oracle_grads(case)
    tower = sorted(set(nt) - set(nf))
    assert tower and all(n.startswith(VT) for n in tower) and all(g32[n] is not None for n in tower)
    check_grads(nt, g32, gemu, tower, case)
    # ---- the never-evaluated layer and post_layernorm: no parameter, no gradient in the oracle either, unchanged by a step
    skipped = unevaluated(tn.W)
    assert skipped and not (skipped & set(nt)) and all(g32[n] is None for n in skipped)
    out = tn.eng.optimizer_step(OPT["lr"], OPT["beta1"], OPT["beta2"], OPT["eps"], OPT["weight_decay"], OPT["max_grad_norm"])
    torch.cuda.synchronize()
    total = math.sqrt(sum(float((g.double() ** 2).sum()) for g in g32.values() if g is not None))
    assert abs(float(out[0]) - total) < 2e-2 * total, (float(out[0]), total)
    for n in skipped:
        assert torch.equal(tn.eng.vision_sd[n].cpu(), tn.W[n].bfloat16()), n
    # every tower matrix moved (a LayerNorm weight near 1 need not: lr = 1e-3 is below half a bf16 ulp of 1, its step stays in the master copy)
    mats = [n for n in tower if tn.W[n].dim() >= 2]
    moved = [n for n in mats if not torch.equal(tn.model.state_dict()[n].cpu().reshape(-1), tn.W[n].bfloat16().reshape(-1))]
    assert len(mats) >= 4 * (tn.cfg["vit_layers"] - 1) + 2 and len(moved) == len(mats), sorted(set(mats) - set(moved))
    # the decay split is HF's
    L = tn.eng.layout
    for hf, nme, r0, rows_ in L.hf_names():
        if hf.startswith(VT):
            assert (L.offset[nme] >= L.n_decay) == O.is_no_decay(hf), hf


@pytest.mark.parametrize("case", CASES)
def test_two_step_trajectory_reference_pass_and_resume(gpu, case, tmp_path):
    a = build(case, True, tmp_path)
    a.eng.init_optimizer()
    pv = a.batch["img_input_dict"]["pixel_values"]
    if case == "llava_hipsmall":
        feat = lambda b, tower: b.eng.vision_features(pv, tower=tower).clone()                                                  # noqa: E731
    else:
        sizes = a.batch["img_input_dict"]["image_sizes"]
        feat = lambda b, tower: b.eng.anyres_vision_features(pv, sizes, 1, tower=tower)[0].clone()                              # noqa: E731
    with torch.no_grad():
        ref1 = [x.clone() for x in a.tr.concatenated_forward(a.ref, a.batch)[:2]]
    f1 = feat(a, a.eng.tower)
    fr1 = feat(a, None)                                                # the initial tower, which the reference pass runs
    assert torch.equal(f1, fr1)                                        # before the first step the two towers are the same weights
    losses = [float(step(a)[0])]
    ckpt = a.tr.save_checkpoint(1, 1, 0) or os.path.join(str(tmp_path), "checkpoint-1")
    with torch.no_grad():
        ref2 = [x.clone() for x in a.tr.concatenated_forward(a.ref, a.batch)[:2]]
    f2 = feat(a, a.eng.tower)
    losses.append(float(step(a)[0]))
    # ---- the reference tower did not move: the reference log-probs of step 2 are the bits of step 1; the policy's features moved
    for x, y in zip(ref1, ref2):
        assert torch.equal(x, y)
    assert not torch.equal(f1, f2)
    a.eng._vit_cache = None
    assert torch.equal(feat(a, None), fr1)
    assert a.model.get_vision_tower() is a.eng.tower and a.ref.get_vision_tower() is a.eng.vision
    with pytest.raises(ValueError, match="train_vision_tower"):      # under LoRA the tower is frozen: a model laid out to train it refuses adapters
        a.eng.enable_lora(8, 16.0)
    # ---- the oracle trajectory the way the HIP path stores things (test_training_trajectory_tracks_oracle), tower included
    names = O.trainable_names(a.W, freeze_vision_tower=False)
    master, Wr16, state, ora = bf(a.W), bf(a.W_ref), {}, []
    for _ in range(2):
        leaves = {k: master[k].bfloat16().float().requires_grad_(True) for k in names}
        Wp = bf(master)
        Wp.update(leaves)
        loss, _ = O.compute_loss(Wp, Wr16, a.cfg, a.batch, a.cfg["beta"], emulate_bf16=EMU)
        loss.backward()
        grads = {k: leaves[k].grad for k in names if leaves[k].grad is not None}
        O.clip_grad_norm_(grads, OPT["max_grad_norm"])
        with torch.no_grad():
            O.adamw_step(master, grads, state, OPT["lr"], OPT["beta1"], OPT["beta2"], OPT["eps"], OPT["weight_decay"])
        ora.append(float(loss))
    print(f"[{case}] losses hip {losses} oracle {ora}")
    assert losses[1] < losses[0]
    for h, r in zip(losses, ora):
        assert abs(h - r) < 3e-2, (losses, ora)
    new = a.model.state_dict()
    for part, keys in (("all", list(grads)), ("tower", [k for k in grads if k.startswith(VT)])):
        num = den = dot = 0.0
        for k in keys:
            dh = new[k].float().cpu().reshape(-1) - a.W[k].bfloat16().float().reshape(-1)
            dr = (master[k] - a.W[k].bfloat16().float()).reshape(-1)
            num += float((dh * dh).sum()); den += float((dr * dr).sum()); dot += float((dh * dr).sum())
        cos = dot / math.sqrt(num * den)
        print(f"[{case}] update direction ({part}): cosine {cos:.4f} norm ratio {math.sqrt(num / den):.4f}")
        assert cos > 0.9 and 0.8 < math.sqrt(num / den) < 1.25, (part, cos, math.sqrt(num / den))
    # ---- the checkpoint holds a moved tower next to the untouched unevaluated tensors, and resuming from it lands on the same bits
    from safetensors.torch import load_file
    saved = {}
    for fn in os.listdir(ckpt):
        if fn.startswith("model") and fn.endswith(".safetensors"):
            saved.update(load_file(os.path.join(ckpt, fn)))
    for n in a.W:
        if n.startswith(VT):
            same = torch.equal(saved[n].reshape(-1), a.W[n].bfloat16().reshape(-1))
            if n in unevaluated(a.W):
                assert same, n
            elif a.W[n].dim() >= 2:          # (a LayerNorm weight near 1 moves in the fp32 master copy only at this learning rate)
                assert not same, n
    b = build(case, True, tmp_path)
    b.eng.init_optimizer()
    b.tr.load_checkpoint(ckpt)
    loss_b, _ = step(b)
    assert float(loss_b) == losses[1]
    assert torch.equal(b.eng.policy.flat.view(torch.int16), a.eng.policy.flat.view(torch.int16))
    assert torch.equal(b.eng.master, a.eng.master)


def test_sft_step_with_a_trainable_tower(gpu):
    """one SFT step: every gradient, the tower's included, against autograd of the oracle's cross-entropy"""
    from tests.test_hip_sft import TOL_CE, ref_ce, sft_inputs, sft_trainer
    from vlrlhf.models.Llava import LlavaForRL
    z, cfg, W, W_ref, batch, rows = load_case("llava_hipsmall")
    inp = sft_inputs(cfg, batch, gpu)
    cpu = {k: v.cpu() for k, v in inp.items()}
    names = O.trainable_names(W, freeze_vision_tower=False)
    res = []
    for emu in (False, EMU):
        leaves = {k: W[k].bfloat16().float().requires_grad_(True) for k in names}
        logits, mlabels, aux = O.llava_forward(leaves, cfg, cpu["input_ids"], cpu["attention_mask"], cpu["labels"], cpu["pixel_values"].float(),
                                               emulate_bf16=emu)
        loss = ref_ce(logits, mlabels, aux["mask"])
        loss.backward()
        res.append((float(loss), {k: v.grad for k, v in leaves.items()}))
    (l32, g32), (_, gemu) = res
    model = LlavaForRL.from_state_dict(dict(cfg, train_vision_tower=True), W)
    tr = sft_trainer(model, cfg)
    model.engine.init_optimizer()
    loss = tr.training_step(model, inp)
    torch.cuda.synchronize()
    assert abs(float(loss) - l32) < TOL_CE, (float(loss), l32)
    named = dict(model.named_parameters())
    assert set(named) == set(names) - unevaluated(W)
    check_grads(named, g32, gemu, sorted(named), "sft")


def test_dpo_entry_point_with_the_flag_trains_and_saves_the_tower(tmp_path):
    """`python -m vlrlhf.dpo ... --freeze_vision_tower False` on an on-disk LLaVA checkpoint: the loader builds the model with a
    trainable tower, the run trains, and the saved model holds a tower that moved (the unevaluated tensors did not) and reloads"""
    from safetensors.torch import load_file
    from tests.golden_util import write_tiny_checkpoint
    from tests.test_entrypoint_gpu import _args
    from vlrlhf import dpo
    from vlrlhf.models.Llava import LlavaForRL
    ckpt, out = str(tmp_path / "ckpt"), str(tmp_path / "out")
    cfg, W = write_tiny_checkpoint(ckpt)
    tr = dpo.main(_args(ckpt, out, freeze_vision_tower="False", max_steps=2, logging_steps=1, learning_rate=1e-3))
    eng = tr.model.engine
    assert eng.train_vision and all(torch.isfinite(torch.tensor(h["loss"])) for h in tr.log_history if "loss" in h)
    eng.wait_optimizer()
    torch.cuda.synchronize()
    saved = load_file(os.path.join(out, "model.safetensors"))
    skipped = unevaluated(W)
    tower = [k for k in W if k.startswith(VT)]
    assert tower and skipped and set(tower) <= set(saved)
    for k in tower:
        same = torch.equal(saved[k].float().reshape(-1), W[k].float().reshape(-1))
        if k in skipped:
            assert same, k
        elif W[k].dim() >= 2:
            assert not same, k
    m2 = LlavaForRL.from_pretrained(out, train_vision_tower=True)
    assert torch.equal(m2.engine.policy.flat, eng.policy.flat)
    # the default load of the same directory keeps that tower frozen: it is the one the forward runs
    m3 = LlavaForRL.from_pretrained(out)
    assert not m3.engine.train_vision and torch.equal(m3.engine.vision.patch_w, m2.engine.tower.patch_w)
