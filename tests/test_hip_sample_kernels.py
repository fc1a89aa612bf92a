"""vlr_sample_tokens (csrc/sample.hip) against the host reference of tests/sample_ref.py: kept masks bit for bit (the golden's of
transformers' warpers among them), tokens equal wherever the reference can decide the draw, log-probs within the derived bound, two calls
bit-identical, nothing written outside its place.  tests/test_sample_checker_host.py shows that the checker flags planted faults and that
the inputs used here are decidable.  Needs a real MI355X:  pytest -m gpu"""
import json
import os

import numpy as np
import pytest
import torch

from tests import sample_ref as SR

pytestmark = pytest.mark.gpu

from tests.test_hip_e2e import gpu  # noqa: E402,F401

SENT_I, SENT_F, SENT_B = -77, -7.5, 0x5A
CASES = SR.kernel_cases()


def run_kernel(hip, kw, ld=None, unfinished=None, finish_step=None, row_ids=None, eos=(), want_kept=True, tail=3):
    """one launch on sentinel-filled buffers with `tail` spare rows -> dict of numpy arrays (check_sample's `out`) + the raw tensors"""
    x = np.asarray(kw["logits"], dtype=np.float32)
    B, V = x.shape
    ld = ld or V
    full = torch.full((B, ld), 123.0, dtype=torch.float32)
    full[:, :V] = torch.from_numpy(x)
    logits = full.cuda()
    before = logits.clone()
    step, out_ld = int(kw.get("step", 0)), int(kw.get("step", 0)) + 3
    unf = torch.full((B + tail,), SENT_B, dtype=torch.uint8)
    unf[:B] = 1 if unfinished is None else torch.as_tensor(np.asarray(unfinished), dtype=torch.uint8)
    fin = torch.full((B + tail,), SENT_I, dtype=torch.int32)
    if finish_step is not None:
        fin[:B] = torch.as_tensor(np.asarray(finish_step), dtype=torch.int32)
    unf, fin = unf.cuda(), fin.cuda()
    nxt = torch.full((B + tail,), SENT_I, dtype=torch.int32, device="cuda")
    ids = torch.full((B + tail, out_ld), SENT_I, dtype=torch.int64, device="cuda")
    logp = torch.full((B + tail,), SENT_F, dtype=torch.float32, device="cuda")
    kept = torch.full((B + tail, V), SENT_B, dtype=torch.uint8, device="cuda") if want_kept else None
    pr, gen = kw.get("prompt_ids"), kw.get("gen_ids")
    pr_t = torch.as_tensor(np.ascontiguousarray(pr), dtype=torch.int64).cuda() if pr is not None and np.asarray(pr).size else None
    gen_t = torch.as_tensor(np.ascontiguousarray(gen), dtype=torch.int64).cuda() if gen is not None else None
    T = 0 if pr_t is None else pr_t.shape[1]
    eos_t = torch.tensor(list(eos), dtype=torch.int32, device="cuda") if eos else None
    rid_t = torch.as_tensor(np.asarray(row_ids), dtype=torch.int32).cuda() if row_ids is not None else None
    hip.call("vlr_sample_tokens", logits, B, V, ld, int(kw.get("do_sample", True)), float(kw.get("temperature", 1.0)), int(kw.get("top_k", 0)),
             float(kw.get("top_p", 1.0)), float(kw.get("penalty", 1.0)), pr_t, T, T, int(kw.get("prompt_div", 1)), gen_t,
             0 if gen_t is None else gen_t.shape[1], int(kw.get("n_gen", 0)), eos_t, len(eos), int(kw.get("pad", 0)), int(kw.get("seed", 0)),
             int(kw.get("call", 0)), step, rid_t, unf, nxt, ids, out_ld, logp, fin, kept)
    torch.cuda.synchronize()
    assert torch.equal(logits, before), "the logits were written"
    assert bool((unf[B:] == SENT_B).all()) and bool((fin[B:] == SENT_I).all()) and bool((nxt[B:] == SENT_I).all())
    assert bool((logp[B:] == SENT_F).all()) and bool((ids[B:] == SENT_I).all())
    assert bool((ids[:B, :step] == SENT_I).all()) and bool((ids[:B, step + 1:] == SENT_I).all())
    assert torch.equal(ids[:B, step], nxt[:B].long())
    if kept is not None:
        assert bool((kept[B:] == SENT_B).all())
    raw = (unf.cpu(), nxt.cpu(), ids.cpu(), logp.cpu(), fin.cpu(), None if kept is None else kept.cpu())
    out = dict(tok=raw[1][:B].numpy(), logp=raw[3][:B].numpy(), unfinished=raw[0][:B].numpy(), finish_step=raw[4][:B].numpy(),
               kept=None if kept is None else raw[5][:B].numpy())
    return out, raw


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_sample_tokens_against_reference(gpu, c):
    from vlrlhf import _hip as hip
    kw, ref = SR.make_case(c)
    ref = SR.sample_ref(**kw, finish_step=np.full(c["B"], SENT_I))
    out, raw = run_kernel(hip, kw, ld=c["ld"])
    _, again = run_kernel(hip, kw, ld=c["ld"])
    assert _same(raw, again)                                   # fixed reduction order, counter-based draw: the same bits
    assert np.array_equal(out["kept"], ref["kept"])            # decidable by construction (make_case): bit-equal, no waiver
    fails, worst, waived = SR.check_sample(out, ref)
    print(f"[sample] {c['name']} kept/row {ref['kept'].sum(1)[:4]} worst logp err/bound {worst:.3f} waived {waived}")
    assert fails == [], fails
    assert waived <= c["B"] // 1000
    nokept, _ = run_kernel(hip, kw, ld=c["ld"], want_kept=False)      # the production call: kept = NULL
    assert np.array_equal(nokept["tok"], out["tok"]) and np.array_equal(nokept["logp"], out["logp"])


def test_golden_kept_masks(gpu):
    """the 8 cases x 6 rows of transformers' own warpers (tests/golden/sampling_warpers.json): the kept masks bit for bit"""
    from vlrlhf import _hip as hip
    d = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "sampling_warpers.json")))
    x = np.array(d["logits"], dtype=np.float32)
    assert len(d["cases"]) == 8 and x.shape[0] == 6
    for n, c in enumerate(d["cases"]):
        kw = dict(logits=x, temperature=c["temperature"], top_k=c["top_k"], top_p=c["top_p"], seed=11, call=n, step=1)
        out, _ = run_kernel(hip, kw, ld=x.shape[1] + 4)
        assert np.array_equal(out["kept"], np.array(c["kept"], dtype=np.uint8)), (n, c["temperature"], c["top_k"], c["top_p"])
        fails, _, waived = SR.check_sample(out, SR.sample_ref(**kw, finish_step=np.full(6, SENT_I)))
        assert fails == [] and waived == 0, fails


def test_top_k_1_is_greedy_is_argmax(gpu):
    from vlrlhf import _hip as hip
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((3, 4099)) * 3).astype(np.float32)
    a, _ = run_kernel(hip, dict(logits=x, do_sample=True, top_k=1, temperature=0.5, seed=9, step=2), ld=4100)
    b, _ = run_kernel(hip, dict(logits=x, do_sample=False, step=2), ld=4100)
    assert np.array_equal(a["tok"], x.argmax(1)) and np.array_equal(b["tok"], x.argmax(1))
    assert bool((a["logp"] == 0).all())                         # one survivor: log 1
    assert bool((a["kept"].sum(1) == 1).all()) and bool((b["kept"] == 1).all())


@pytest.mark.parametrize("n_eos", [1, 8])
def test_eos_and_finished_rows(gpu, n_eos):
    """rows 0 / 2 draw an eos id (top_k = 1 pins the token), row 1 does not, row 3 came in finished"""
    from vlrlhf import _hip as hip
    rng = np.random.default_rng(17)
    V, pad = 65, 63
    x = (rng.standard_normal((4, V)) * 3).astype(np.float32)
    x[0, 10], x[1, 20], x[2, 30] = 20.0, 20.0, 20.0
    am = np.array([10, 20, 30, int(x[3].argmax())])
    others = [i for i in range(V) if i not in set(am.tolist())]
    eos = [int(am[0])] if n_eos == 1 else others[:3] + [int(am[2])] + others[3:6] + [int(am[0])]
    kw = dict(logits=x, do_sample=True, top_k=1, seed=3, step=4, pad=pad)
    unf, fin = np.array([1, 1, 1, 0]), np.array([SENT_I, SENT_I, SENT_I, 2])
    out, _ = run_kernel(hip, kw, ld=68, unfinished=unf, finish_step=fin, eos=eos)
    ref = SR.sample_ref(**kw, eos=eos, unfinished=unf, finish_step=fin)
    fails, _, waived = SR.check_sample(dict(out, kept=None), ref)
    assert fails == [] and waived == 0, fails
    want_unf = [0, 1, 0 if n_eos == 8 else 1, 0]
    assert out["unfinished"].tolist() == want_unf
    assert out["finish_step"].tolist() == [4, SENT_I, 4 if n_eos == 8 else SENT_I, 2]
    assert out["tok"][3] == pad and out["logp"][3] == 0.0 and out["tok"][0] == am[0]      # the eos itself is emitted
    assert bool((out["kept"][3] == SENT_B).all())               # a finished row draws nothing and writes no mask


def test_row_ids_follow_the_id_not_the_position(gpu):
    """the same logits in every row: a row's token is a function of its row_id alone - permuting the ids permutes the tokens, a sub-batch
    draws what the full batch drew, and NULL means 0 .. B - 1"""
    from vlrlhf import _hip as hip
    rng = np.random.default_rng(23)
    B, V = 12, 1025
    x = np.repeat((rng.standard_normal((1, V)) * 2).astype(np.float32), B, 0)
    kw = dict(logits=x, temperature=1.0, top_k=0, top_p=1.0, seed=77, call=1, step=9)
    base, _ = run_kernel(hip, kw, want_kept=False)
    assert len(set(base["tok"].tolist())) > 3                   # the rows do differ
    perm = rng.permutation(B)
    got, _ = run_kernel(hip, kw, row_ids=perm, want_kept=False)
    assert np.array_equal(got["tok"], base["tok"][perm]) and np.array_equal(got["logp"], base["logp"][perm])
    sub, _ = run_kernel(hip, dict(kw, logits=x[:3]), row_ids=[7, 2, 11], want_kept=False)
    assert np.array_equal(sub["tok"], base["tok"][[7, 2, 11]])
    ref = SR.sample_ref(**kw, row_ids=perm, finish_step=np.full(B, SENT_I))
    fails, _, waived = SR.check_sample(got, ref)
    assert fails == [] and waived == 0, fails
    other, _ = run_kernel(hip, dict(kw, step=10), want_kept=False)
    assert not np.array_equal(other["tok"], base["tok"])        # another step, another draw


def test_distribution_chi_square(gpu):
    """V = 8, fixed logits, 50 000 rows with distinct row_id in one launch under (T 0.7, k 5, p 0.9): the token counts against the fp64
    softmax over the kept set, rejected above the 1 - 1e-6 quantile of chi-square with (kept - 1) degrees of freedom (sample_ref.chi2_sf, the
    closed form).  The seed is fixed, so the test is deterministic."""
    from vlrlhf import _hip as hip
    B, V = 50000, 8
    row = np.array([1.2, -0.3, 0.8, 2.0, -1.5, 0.1, 1.9, 0.5], dtype=np.float32)
    kw = dict(logits=np.repeat(row[None], B, 0), temperature=0.7, top_k=5, top_p=0.9, seed=20240607, call=0, step=0)
    out, _ = run_kernel(hip, kw, ld=8)
    ref = SR.sample_ref(**dict(kw, logits=row[None]))
    assert not ref["kept_undecidable"].any()
    kept = ref["kept"][0].astype(bool)
    assert bool((out["kept"] == ref["kept"][0]).all())
    counts = np.bincount(out["tok"], minlength=V)
    assert counts[~kept].sum() == 0                             # nothing is ever drawn outside the kept set
    z = ref["z"][0].astype(np.float64)
    p = np.where(kept, np.exp(z - ref["lse"][0]), 0.0)
    chi2 = float((((counts - B * p) ** 2)[kept] / (B * p[kept])).sum())
    df = int(kept.sum()) - 1
    print(f"[sample] chi-square {chi2:.2f} at {df} degrees of freedom, kept {kept.astype(int)}, counts {counts}")
    assert df >= 1 and SR.chi2_sf(chi2, df) >= 1e-6
    want = np.float32(z - ref["lse"][0])[out["tok"]]
    assert np.abs(out["logp"] - want).max() < 1e-5


def test_argument_ranges_are_refused(gpu):
    from vlrlhf import _hip as hip
    x = np.zeros((2, 16), dtype=np.float32)
    for bad in (dict(temperature=0.0), dict(top_p=0.0), dict(top_p=1.5), dict(penalty=0.0), dict(penalty=-1.0)):
        with pytest.raises(ValueError, match="vlr_sample_tokens"):
            run_kernel(hip, dict(logits=x, **bad))
    with pytest.raises(ValueError, match="n_eos"):
        run_kernel(hip, dict(logits=x), eos=list(range(9)))
