"""tests/sample_ref.py checks itself on the CPU: the checker accepts the reference's own outputs (also after an fp32 rounding of the
log-probs), flags every planted fault, and the inputs the GPU tests use satisfy the conditions those tests rely on - no token within eps_p of
a top-p cut, at most 1 draw in 1000 with its runner-up within delta, and the reference's top-p rule reproduces the kept masks transformers'
own warpers produced (tests/golden/sampling_warpers.json)."""
import json
import os

import numpy as np
import pytest

from tests import sample_ref as SR


def _as_out(ref):
    return dict(tok=ref["tok"].copy(), logp=ref["logp"].astype(np.float32), kept=ref["kept"].copy(), unfinished=ref["unfinished"].copy(),
                finish_step=ref["finish_step"].copy())


def _logits(B, V, seed, quantum=None):
    x = (np.random.default_rng(seed).standard_normal((B, V)) * 3).astype(np.float32)
    return (np.round(x / quantum) * quantum).astype(np.float32) if quantum else x


def _order_sensitive_pair():
    """(a, b, pen, T): fl(fl(a / pen) / T) != fl(fl(a / T) / pen), and fl(b / T) equals the first - the penalised token ties with b at the
    top only when the penalty comes BEFORE the temperature"""
    pen, T = np.float32(1.3), np.float32(0.7)
    rng = np.random.default_rng(3)
    for a in (rng.random(4000) * 4 + 1).astype(np.float32):
        right, wrong = (a / pen) / T, (a / T) / pen
        if right == wrong:
            continue
        for b in np.nextafter(right * T, [np.float32(-np.inf), np.float32(np.inf), right * T]).astype(np.float32):
            if b / T == right:
                return float(a), float(b), float(pen), float(T)
    raise AssertionError("no order-sensitive pair found")


def _fault_inputs():
    a, b, pen, T = _order_sensitive_pair()
    x_order = np.full((2, 16), -5.0, dtype=np.float32)
    x_order[:, 3], x_order[:, 9] = a, b
    x_dup = _logits(4, 33, 5)
    x_dup[:, 7] = 9.0
    eosx = _logits(4, 33, 6)
    eosx[:, 4] = 30.0
    return {
        "topk_off_by_one": dict(logits=_logits(4, 65, 1), top_k=5),
        "tie_dropped": dict(logits=_logits(4, 65, 2, quantum=2.0), top_k=2),
        "topp_le": dict(logits=_logits(4, 65, 3), top_k=0, top_p=0.5),
        "dup_twice": dict(logits=x_dup, penalty=1.5, prompt_ids=np.array([[7, 7, 2]] * 4), gen_ids=np.zeros((4, 1), dtype=np.int64), n_gen=0),
        "pen_after_temp": dict(logits=x_order, penalty=pen, temperature=T, top_k=1, prompt_ids=np.array([[3]] * 2)),
        "philox_word_shift": dict(logits=_logits(16, 65, 4), seed=99),
        "rowid_from_position": dict(logits=np.repeat(_logits(1, 65, 7), 16, 0), seed=5, row_ids=np.arange(16)[::-1].copy()),
        "finished_not_padded": dict(logits=_logits(4, 33, 8), unfinished=np.array([1, 0, 1, 0]), pad=1),
        "eos_not_clearing": dict(logits=eosx, top_k=1, eos=(4,)),
        "logp_unfiltered": dict(logits=_logits(4, 65, 9), top_k=5),
    }


FAULTS = _fault_inputs()


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_checker_flags_planted_fault(fault):
    kw = dict(seed=1, call=2, step=3, finish_step=np.full(FAULTS[fault]["logits"].shape[0], -1))
    kw.update(FAULTS[fault])
    ref = SR.sample_ref(**kw)
    assert not ref["kept_undecidable"].any()
    fails, worst, waived = SR.check_sample(_as_out(ref), ref)
    assert fails == [] and waived == 0 and worst < 1, (fails, worst)       # the reference rounded to fp32 passes its own check
    bad = SR.sample_ref(**kw, fault=fault)
    fails, _, _ = SR.check_sample(_as_out(bad), ref)
    assert fails, f"the checker let the planted fault {fault} pass"


def test_checker_waives_only_undecidable_draws():
    """a token other than the reference's is accepted only when the two best scores lie within delta"""
    x = _logits(8, 65, 11)
    ref = SR.sample_ref(x, seed=4, finish_step=np.full(8, -1))
    out = _as_out(ref)
    second = np.argsort(ref["z"].astype(np.float64) + SR.gumbel(65, 4, 0, 0, np.arange(8)), axis=1)[:, -2]
    out["tok"][0] = second[0]
    out["logp"][0] = np.float32(ref["z"][0, second[0]] - ref["lse"][0])
    fails, _, waived = SR.check_sample(out, ref)
    assert len(fails) == 1 and waived == 0
    ref["gap"][0] = 0.0                                       # the same row, had its two scores tied
    fails, _, waived = SR.check_sample(out, ref)
    assert fails == [] and waived == 1
    out2 = _as_out(SR.sample_ref(x, seed=4, top_k=3, finish_step=np.full(8, -1)))
    ref2 = SR.sample_ref(x, seed=4, top_k=3, finish_step=np.full(8, -1))
    out2["tok"][2] = int(np.argmin(ref2["kept"][2]))          # a token outside the kept set is never waived
    ref2["gap"][2] = 0.0
    assert SR.check_sample(out2, ref2)[0]


def test_derived_quantities():
    assert SR.depth(1) == 4 + 39 and SR.depth(4096) == 43 and SR.depth(4097) == 47 and SR.depth(151936) == 4 * 38 + 39
    assert SR.eps_p(151936) < 8.9e-4 / 10                     # an order below the golden's smallest |mass - top_p|
    assert 1e-6 < SR.delta(50.0) < 1e-4
    g = SR.gumbel(4096, 7, 1, 2, [0, 1])
    assert g.min() >= -np.log(25 * np.log(2.0)) - 1e-9 and g.max() <= SR.GUMBEL_MAX + 1e-6
    assert abs(g.mean() - 0.5772) < 0.05                      # Euler-Mascheroni: a Gumbel variate's mean
    assert SR.chi2_sf(27.631, 2) == pytest.approx(1e-6, rel=1e-3) and SR.chi2_sf(30.665, 3) == pytest.approx(1e-6, rel=2e-3)


def test_reference_rule_reproduces_the_golden_masks():
    d = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "sampling_warpers.json")))
    x = np.array(d["logits"], dtype=np.float32)
    rows = 0
    for c in d["cases"]:
        ref = SR.sample_ref(x, temperature=c["temperature"], top_k=c["top_k"], top_p=c["top_p"])
        assert np.array_equal(ref["kept"], np.array(c["kept"], dtype=np.uint8)), c
        assert not ref["kept_undecidable"].any()              # what tests/test_hip_sample_kernels.py::test_golden_kept_masks relies on
        rows += x.shape[0]
    assert rows == 48


def test_gpu_test_inputs_are_decidable():
    """every case of the kernel test: make_case settled on logits with no kept bit inside eps_p and no draw inside delta"""
    for c in SR.kernel_cases():
        kw, ref = SR.make_case(c)
        zmax = float(np.abs(ref["z"][np.isfinite(ref["z"])]).max())
        assert not ref["kept_undecidable"].any(), c["name"]
        assert int((ref["gap"] < SR.delta(zmax)).sum()) <= c["B"] // 1000, c["name"]
        assert np.isfinite(ref["logp"]).all(), c["name"]


def test_share_of_undecidable_draws():
    """V = 8, 200 000 draws: the share whose top-two gap is below the derived delta is at most 1 in 1000 (with a 1e-4 gap it measured
    1.2e-4; delta is a few 1e-5)"""
    row = np.array([1.2, -0.3, 0.8, 2.0, -1.5, 0.1, 1.9, 0.5], dtype=np.float32)
    ref = SR.sample_ref(np.repeat(row[None], 200000, 0), temperature=0.7, top_k=5, top_p=0.9, seed=20240607)
    share = float((ref["gap"] < SR.delta(float(np.abs(ref["z"]).max()))).mean())
    print(f"share of draws within delta: {share:.2e}")
    assert share <= 1e-3
    assert not ref["kept_undecidable"][:1].any()              # the chi-square test's row
