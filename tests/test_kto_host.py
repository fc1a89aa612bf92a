"""KTO without a GPU: the KL shift of the collator, the batch-of-one refusal, every refusal of VLKTOTrainer and vlrlhf/kto.py by name, the
weight-balance warning on both sides of [1, 4/3], the unpaired datasets, the registry, the script arguments, and the argument errors of
vlr_kto_loss."""
import json
import os
from types import SimpleNamespace

import pytest
import torch

from tests.golden_util import GOLDEN

PAD = -100


def _row(prompt, answer, label, img):
    ids = list(prompt) + list(answer)
    return dict(completion_input_ids=ids, completion_attention_mask=[1] * len(ids), completion_labels=[PAD] * len(prompt) + list(answer),
                label=label, img_path=img)


def _collator(**kw):
    from vlrlhf.base.collator import VLDPODataCollatorWithPadding, VLKTODataCollatorWithPadding
    return VLKTODataCollatorWithPadding(VLDPODataCollatorWithPadding(pad_token_id=0, label_pad_token_id=PAD), **kw)


ROWS = [_row([1, 11, 12], [101, 102], True, "a.jpg"), _row([1, 21], [201, 202, 203, 204], False, "b.jpg"),
        _row([1, 31, 32, 33], [301], True, "c.jpg")]


# ------------------------------------------------------------------------------------------------------------ the collator
def test_kl_rows_carry_the_previous_completion_prompts_and_images_stay():
    out = _collator()(ROWS)
    B = len(ROWS)
    assert out["img_path"] == ["a.jpg", "b.jpg", "c.jpg"] and out["kto_label"].tolist() == [1, 0, 1] and out["kto_label"].dtype == torch.uint8
    prompts = [[1, 11, 12], [1, 21], [1, 31, 32, 33]]
    answers = [[101, 102], [201, 202, 203, 204], [301]]
    for i in range(B):
        main = prompts[i] + answers[i]
        assert out["chosen_input_ids"][i, : len(main)].tolist() == main and bool((out["chosen_input_ids"][i, len(main):] == 0).all())
        assert out["chosen_labels"][i, : len(main)].tolist() == [PAD] * len(prompts[i]) + answers[i]
        kl = prompts[i] + answers[(i - 1) % B]      # row i: prompt i with completion i - 1; row 0 carries the last one
        assert out["rejected_input_ids"][i, : len(kl)].tolist() == kl and bool((out["rejected_input_ids"][i, len(kl):] == 0).all())
        assert out["rejected_labels"][i, : len(kl)].tolist() == [PAD] * len(prompts[i]) + answers[(i - 1) % B]
        assert bool((out["rejected_labels"][i, len(kl):] == PAD).all())
        assert out["rejected_attention_mask"][i].tolist() == [1] * len(kl) + [0] * (out["rejected_attention_mask"].shape[1] - len(kl))
    # both halves have B rows: the pair contract of a [chosen ; rejected] batch
    assert out["chosen_input_ids"].shape[0] == out["rejected_input_ids"].shape[0] == B


def test_kl_rows_keep_the_prompt_and_cut_the_completion_to_fit():
    out = _collator(max_length=6, max_prompt_length=3)(ROWS)
    # row 2: prompt of 4 (above max_prompt_length: it stays, the image tokens with it) + completion 1 of 4 = 8 > 6: the completion is cut to 6 - 4
    assert out["rejected_input_ids"][2].tolist()[:6] == [1, 31, 32, 33, 201, 202] and out["rejected_labels"][2].tolist()[:6] == [PAD] * 4 + [201, 202]
    # row 1: prompt of 2 + completion 0 of 2 fits: untouched
    assert out["rejected_input_ids"][1].tolist()[:4] == [1, 21, 101, 102]
    # a prompt below max_prompt_length: the completion is cut as the tokeniser cuts an answer, to max_length - max_prompt_length
    rows = [_row([1, 2], [5, 6, 7, 8, 9], True, "a"), _row([1, 3], [4], False, "b")]
    out = _collator(max_length=6, max_prompt_length=3)(rows)
    assert out["rejected_input_ids"][1].tolist() == [1, 3, 5, 6, 7] and out["rejected_labels"][1].tolist() == [PAD, PAD, 5, 6, 7]
    # a prompt that fills max_length alone: one completion token stays
    out = _collator(max_length=4, max_prompt_length=2)(ROWS)
    assert out["rejected_input_ids"][2].tolist()[:5] == [1, 31, 32, 33, 201]
    # the main rows are never touched by the collator
    assert out["chosen_input_ids"][1].tolist()[:6] == [1, 21, 201, 202, 203, 204]


def test_a_batch_of_one_row_is_refused():
    from vlrlhf.base.trainer import KTOConfig, VLKTOTrainer
    with pytest.raises(ValueError, match="per_device_train_batch_size > 1"):
        _collator()(ROWS[:1])
    with pytest.raises(ValueError, match="per_device_train_batch_size > 1"):
        VLKTOTrainer(SimpleNamespace(), SimpleNamespace(), KTOConfig(per_device_train_batch_size=1))
    # a trailing batch of one row is left out of the epoch, and the loop counts the batches that way
    tr = VLKTOTrainer(SimpleNamespace(), SimpleNamespace(), KTOConfig(per_device_train_batch_size=2, dataloader_prefetch=0), train_dataset=ROWS,
                      data_collator=_collator())
    batches = list(tr._train_row_batches(0))
    assert [len(b) for b in batches] == [2] and tr._batches_per_epoch() == 1


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("bs", [2, 4])
@pytest.mark.parametrize("n", [4, 5, 7, 9])
def test_batches_of_an_epoch_and_resume_skip_agree(n, bs, drop_last):
    """the loop resumes by (epoch, batches to skip) = divmod(micro_step, _batches_per_epoch()): the count must be the number of batches an
    epoch yields, for every epoch, and the batch left out (a trailing one of one row) must be the last, so that skipping k batches of the
    filtered epoch lands where the uninterrupted run stood - also across an epoch boundary with an odd row count"""
    import itertools
    from vlrlhf.base.trainer import KTOConfig, VLKTOTrainer, VLTrainerLoop
    rows = [_row([1, i], [100 + i], i % 2 == 0, f"{i}.jpg") for i in range(n)]
    tr = VLKTOTrainer(SimpleNamespace(), SimpleNamespace(), KTOConfig(per_device_train_batch_size=bs, dataloader_drop_last=drop_last, seed=7),
                      train_dataset=rows)
    per = tr._batches_per_epoch()
    micro = []      # the uninterrupted run: (epoch, batch) of every micro-step over three epochs
    for ep in range(3):
        got = list(tr._train_row_batches(ep))
        parent = list(VLTrainerLoop._train_row_batches(tr, ep))
        assert len(got) == per and all(len(b) >= 2 for b in got)
        assert got == parent[: len(got)] and len(parent) - len(got) <= 1      # only a LAST batch is ever left out
        micro += [(ep, b) for b in got]
    for m in range(len(micro)):      # resumed at micro-step m: the batches from there on are the uninterrupted run's
        ep, skip = divmod(m, per)
        rest = list(itertools.islice(tr._train_row_batches(ep), skip, None))
        assert rest[0] == micro[m][1] and micro[m][0] == ep


# ------------------------------------------------------------------------------------------------------------ refusals
def test_trainer_refusals_by_name(monkeypatch):
    from vlrlhf.base import trainer as T
    cfg = T.KTOConfig(per_device_train_batch_size=2)
    plain, ref = SimpleNamespace(), SimpleNamespace()
    with pytest.raises(ValueError, match="needs a model"):
        T.VLKTOTrainer(None, ref, cfg)
    with pytest.raises(NotImplementedError, match="precompute_ref_log_probs"):
        T.VLKTOTrainer(plain, ref, cfg, precompute_ref_log_probs=True)
    with pytest.raises(NotImplementedError, match="precompute_ref_log_probs"):
        T.VLKTOTrainer(plain, ref, T.KTOConfig(per_device_train_batch_size=2, precompute_ref_log_probs=True))
    with pytest.raises(NotImplementedError, match="reference_free"):
        T.VLKTOTrainer(plain, ref, cfg, reference_free=True)
    with pytest.raises(NotImplementedError, match="q_lora"):
        T.VLKTOTrainer(SimpleNamespace(is_packed=True), ref, cfg)
    with pytest.raises(NotImplementedError, match="freeze_vision_tower False"):
        T.VLKTOTrainer(SimpleNamespace(engine=SimpleNamespace(train_vision=True, dev="cpu")), ref, cfg)
    with pytest.raises(ValueError, match="value head"):
        T.VLKTOTrainer(SimpleNamespace(v_head=object()), ref, cfg)
    monkeypatch.setattr(T, "_world", lambda: 2)
    with pytest.raises(NotImplementedError, match="more than one GPU: trl averages kl across the ranks"):
        T.VLKTOTrainer(plain, ref, cfg)


def test_script_refusals_by_name_and_argument_parsing(monkeypatch):
    from vlrlhf import kto
    s, t, l = kto.parse_args(["--model_name_or_path", "/m", "--beta", "0.25", "--desirable_weight", "1.5", "--undesirable_weight", "0.5",
                              "--per_device_train_batch_size", "8", "--max_length", "256", "--max_prompt_length", "64", "--dataset_name", "kto_json",
                              "--use_lora", "true", "--lora_r", "32", "--eval_strategy", "steps", "--neftune_noise_alpha", "5"])
    assert (t.beta, t.desirable_weight, t.undesirable_weight, t.max_length, t.max_prompt_length) == (0.25, 1.5, 0.5, 256, 64)
    assert s.dataset_name == "kto_json" and s.model_name_or_path == "/m" and t.use_lora and l.lora_r == 32 and t.per_device_train_batch_size == 8
    assert t.evaluation_strategy == "steps" and t.neftune_noise_alpha == 5.0 and s.freeze_vision_tower and not s.reference_free
    d = kto.parse_args([])
    assert (d[1].beta, d[1].desirable_weight, d[1].undesirable_weight, d[0].dataset_name) == (0.1, 1.0, 1.0, "vlfeedback_unpaired")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    kto.check_arguments(s, t, l)
    for argv, exc, msg in ((["--precompute_ref_log_probs", "true"], NotImplementedError, "precompute_ref_log_probs"),
                           (["--reference_free", "true"], NotImplementedError, "reference_free"),
                           (["--use_lora", "true", "--q_lora", "true"], NotImplementedError, "q_lora"),
                           (["--freeze_vision_tower", "False"], NotImplementedError, "freeze_vision_tower False"),
                           (["--per_device_train_batch_size", "1"], ValueError, "per_device_train_batch_size > 1")):
        with pytest.raises(exc, match=msg):
            kto.check_arguments(*kto.parse_args(argv))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="more than one GPU"):
        kto.check_arguments(*kto.parse_args([]))
    from vlrlhf.base.trainer import KTOConfig
    with pytest.raises(ValueError, match="beta"):
        KTOConfig(beta=float("nan"))


# ------------------------------------------------------------------------------------------------------------ the balance warning
@pytest.mark.parametrize("n_d,n_u,w_d,w_u,warns", [
    (4, 4, 1.0, 1.0, False),      # ratio 1: the lower edge
    (4, 3, 1.0, 1.0, False),      # 4/3: the upper edge
    (3, 4, 1.0, 1.0, True),       # 0.75: below
    (4, 2, 1.0, 1.0, True),       # 2: above
    (4, 2, 1.0, 1.6, False),      # 2 / 1.6 = 1.25: the weights bring it back inside
    (2, 4, 2.2, 1.0, False),      # 1.1
    (4, 0, 1.0, 1.0, False),      # one class only: nothing to balance
])
def test_balance_warning(capsys, n_d, n_u, w_d, w_u, warns):
    from vlrlhf.base.trainer import KTOConfig, VLKTOTrainer
    rows = [_row([1, 2], [3], True, "a")] * n_d + [_row([1, 2], [4], False, "b")] * n_u
    tr = VLKTOTrainer(SimpleNamespace(), SimpleNamespace(), KTOConfig(desirable_weight=w_d, undesirable_weight=w_u), train_dataset=rows)
    out = capsys.readouterr().out
    assert (tr.balance_warning is not None) == warns and (("outside [1, 4/3]" in out) == warns)
    if warns:
        assert out.count("\n") == 1 and f"{n_d}" in out and f"{n_u}" in out      # one log line


# ------------------------------------------------------------------------------------------------------------ datasets, registry
def test_unpairing_the_vlfeedback_pairs(tmp_path):
    from vlrlhf.utils.data import DATASET_MAP, unpair, vlfeedback_pairs
    g = json.load(open(os.path.join(GOLDEN, "vlfeedback_pairs.json")))
    s = g["samples"]
    samples = [dict(prompt=s["prompt"][i], img_path=s["img_path"][i], completions=s["completions"][i]) for i in range(len(s["prompt"]))]
    pairs = vlfeedback_pairs(samples, -1)
    rows = unpair(pairs)
    assert len(pairs) >= 2 and len(rows) == 2 * len(pairs)
    for i, p in enumerate(pairs):
        a, b = rows[2 * i], rows[2 * i + 1]
        assert (a["label"], b["label"]) == (True, False) and a["prompt"] == b["prompt"] == p["prompt"] and a["img_path"] == b["img_path"] == p["img_path"]
        assert a["completion"] == p["chosen"] and b["completion"] == p["rejected"] and set(a) == {"prompt", "completion", "label", "img_path"}
    f = tmp_path / "vlf.jsonl"
    f.write_text("\n".join(json.dumps(x) for x in samples))
    got = DATASET_MAP["vlfeedback_unpaired"](SimpleNamespace(data_path=str(f), image_root="/imgs", score_margin=-1))
    assert len(got) == len(rows) and got[0]["img_path"].startswith("/imgs/") and [r["label"] for r in got[:2]] == [True, False]
    # kto_json: rows as they are, labels as booleans or words
    j = tmp_path / "kto.json"
    j.write_text(json.dumps([dict(prompt="p", completion="c", label=True, image="x.jpg"), dict(prompt="p", completion="d", label="false", image="y.jpg")]))
    got = DATASET_MAP["kto_json"](SimpleNamespace(data_path=str(j), image_root="/r"))
    assert got == [dict(prompt="p", completion="c", label=True, img_path="/r/x.jpg"), dict(prompt="p", completion="d", label=False, img_path="/r/y.jpg")]
    syn = DATASET_MAP["synthetic_unpaired"](SimpleNamespace(synthetic_rows=6, synthetic_image_size=28))
    assert len(syn) == 6 and [r["label"] for r in syn] == [True, False] * 3 and syn[0]["prompt"] == syn[1]["prompt"]
    assert "rlhfv_unpaired" in DATASET_MAP


def test_registry_and_exports():
    from vlrlhf.base import KTOConfig, VLKTODataCollatorWithPadding, VLKTOTrainer  # noqa: F401
    from vlrlhf.utils import auto_load as A
    import vlrlhf.models.InternLMXC2 as I
    import vlrlhf.models.Llava as L
    import vlrlhf.models.LlavaNext as N
    import vlrlhf.models.QwenVL as Q
    for pkg, dpo in ((L, L.LlavaDPOTrainer), (N, N.LlavaNextDPOTrainer), (Q, Q.QwenVLDPOTrainer), (I, I.InternLMXC2DPOTrainer)):
        assert issubclass(pkg.kto_core.trainer, VLKTOTrainer) and pkg.kto_core.trainer.dpo_trainer_cls is dpo
        assert pkg.kto_core.dpo_collator is pkg.core_mapper.dpo_collator      # every family VLDPOTrainer takes
    assert hasattr(A, "MyAutoKTOTrainer") and hasattr(A, "MyAutoKTOCollator")


def test_kto_rows_are_tokenised_by_the_family_dpo_tokenize_row():
    """tokenize_row hands prompt + completion to the DPO trainer's tokenize_row as a pair of equal answers and keeps the chosen side"""
    from vlrlhf.base.trainer import KTOConfig, VLKTOTrainer
    seen = []

    class Dpo:
        def tokenize_row(self, feature, model=None):
            seen.append(feature)
            return dict(chosen_input_ids=[1, 2, 3], chosen_attention_mask=[1, 1, 1], chosen_labels=[PAD, 2, 3], rejected_input_ids=[9])

    class K(VLKTOTrainer):
        dpo_trainer_cls = Dpo
    tr = K(SimpleNamespace(), SimpleNamespace(), KTOConfig(), train_dataset=[dict(prompt="p", completion="c", label=1, img_path="i.jpg")] * 2)
    assert seen[0] == dict(prompt="p", chosen="c", rejected="c", img_path="i.jpg")
    assert tr.train_dataset[0] == dict(completion_input_ids=[1, 2, 3], completion_attention_mask=[1, 1, 1], completion_labels=[PAD, 2, 3], label=True,
                                       img_path="i.jpg")


# ------------------------------------------------------------------------------------------------------------ the entry point's argument errors
def test_vlr_kto_loss_is_exported_and_refuses_bad_arguments_without_a_gpu():
    from vlrlhf import _hip
    l = _hip.lib()
    assert "vlr_kto_loss" in _hip.exported_symbols() and _hip.helper("vlr_abi_version") == 9
    p = 0x1000      # never dereferenced: every call below is refused before a launch
    good = [p, p, p, 4, p, p, 4, 0.1, 1.0, 1.0, 1.0, p, p, p, p, None]
    for i, v, msg in ([(i, None, b"null operand") for i in (0, 1, 2, 4, 5, 11, 12, 13, 14)]
                      + [(3, 0, b"bad shape"), (3, (1 << 20) + 1, b"bad shape"), (6, 0, b"bad shape"), (6, (1 << 20) + 1, b"bad shape")]
                      + [(i, float(x), b"not finite") for i in (7, 8, 9, 10) for x in ("nan", "inf", "-inf")]):
        a = list(good)
        a[i] = v
        assert l.vlr_kto_loss(*a) == 1 and msg in l.vlr_last_error(), (i, v, l.vlr_last_error())
