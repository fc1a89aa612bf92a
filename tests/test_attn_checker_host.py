"""The attention checker of tests/attn_ref.py, on the CPU: the kernels' rounding model (emulate_kernel_rounding) passes check_tiles at
the tolerances the GPU parity matrix (tests/test_hip_attention_edges.py) uses, on that matrix's cases with S <= 300, and each of a set
of simulated kernel bugs fails it by at least 3x those tolerances on every case it applies to."""
import math

import pytest
import torch

from tests import attn_ref as A

CASES = A.cases(max_S=300)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_kernel_rounding_model_passes(c):
    q, k, v, do, km = A.make_inputs(c)
    emu = A.emulate_kernel_rounding(q, k, v, km, c.causal, do=do)
    ref = A.ref_attention(q, k, v, km, c.causal, do=do, o_bwd=emu.o)
    A.check_attention(emu, ref, A.TOL[c.group], c.name, fwd_only=not c.bwd)


def _applies(bug, c, km):
    masked = km is not None and bool((km == 0).any())
    if bug == "diag_dropped":
        return c.causal and c.S >= 2
    if bug == "future_key":             # not where the diagonal outscores every other key by ~40: one more key adds e^-40
        return c.causal and c.S >= 2 and c.scores != "spike"
    if bug == "tail_tile_ignored":
        return c.S % A.KV_TILE != 0 and (km is None or bool(km[:, c.S // A.KV_TILE * A.KV_TILE:].any()))
    if bug == "no_rescale":
        return c.scores in ("rising", "spike")
    if bug == "gqa_mod":
        return 1 < c.nkv < c.nh
    if bug == "mask_tile_ignored":
        return masked
    if bug == "dk_scale_tile":          # S = 1: every row sees one key, dK is exactly 0 whatever its scale
        return c.bwd and c.S >= 2
    if bug == "noncausal_as_causal":
        return not c.causal and c.S >= 2
    raise KeyError(bug)


def detection_margin(res, ref, tol, bwd):
    """largest (tile error / tolerance) over the outputs; inf when a structural zero / +inf row is not exact"""
    worst = 0.0
    for n in ("o", "lse", "dq", "dk", "dv") if bwd else ("o", "lse"):
        z = dict(o=ref.zero_q, lse=ref.zero_q, dq=ref.zero_dq, dk=ref.zero_kv, dv=ref.zero_kv)[n]
        x, r = getattr(res, n), getattr(ref, n)
        if bool(z.any()) and bool((x[z].double() != r[z]).any()):
            return math.inf
        worst = max(worst, float(A.tile_errors(x, r).max()) / tol[n])
    return worst


@pytest.mark.parametrize("bug", A.BUGS)
def test_simulated_kernel_bugs_fail_the_checker(bug):
    n, missed = 0, []
    for c in CASES:
        q, k, v, do, km = A.make_inputs(c)
        if not _applies(bug, c, km):
            continue
        n += 1
        bad = A.emulate_kernel_rounding(q, k, v, km, c.causal, do=do, bug=bug)
        ref = A.ref_attention(q, k, v, km, c.causal, do=do, o_bwd=bad.o)
        m = detection_margin(bad, ref, A.TOL[c.group], c.bwd)
        if m < 3.0:
            missed.append(f"{c.name}: {m:.2f}x")
            continue
        with pytest.raises(AssertionError):
            A.check_attention(bad, ref, A.TOL[c.group], c.name, fwd_only=not c.bwd)
    assert not missed, f"{bug}: worst tile error under 3x the tolerance on " + ", ".join(missed)
    assert n >= 3, (bug, n)


def test_checker_reports_the_worst_tile_and_exact_zeros():
    ref = torch.zeros(2, 130, 3, 8, dtype=torch.float64)
    ref[:, 2:] = 1.0
    out = ref.clone()
    out[1, 70, 2, 5] += 0.5                                  # tile 1 of (b = 1, h = 2)
    with pytest.raises(AssertionError, match=r"\(1, 2, 1\)"):
        A.check_tiles(out, ref, 1e-2)
    zero = torch.zeros(2, 130, 3, dtype=torch.bool)
    zero[:, :2] = True
    out = ref.clone()
    out[0, 1, 0, 0] = 1e-30                                  # a structural zero row must be exactly 0
    with pytest.raises(AssertionError, match="exactly 0"):
        A.check_tiles(out, ref, 1e-2, zero=zero)
    lse = torch.full((1, 64, 1), math.inf, dtype=torch.float64)
    with pytest.raises(AssertionError, match=r"\+inf"):
        A.check_tiles(torch.zeros_like(lse), lse, 1e-2, zero=torch.ones(1, 64, 1, dtype=torch.bool))
    out = ref.clone()
    out[0, 129, 0, 0] = float("nan")                         # an unwritten (NaN) row in the last, partial tile
    with pytest.raises(AssertionError, match=r"\(0, 0, 2\)"):
        A.check_tiles(out, ref, 1e-2)
