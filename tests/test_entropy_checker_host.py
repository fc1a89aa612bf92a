"""CPU-only: the checker of the entropy tests (tests/entropy_ref.py) accepts a correct fp32 replay of the partial / fold scheme and flags
every planted fault, so a GPU test that passes it has shown something.  The shapes are those of tests/test_hip_entropy_kernels.py with
the row count of the two large ones cut to the planted rows and a handful of random ones (the scheme is row by row: V and H, which
decide the parts, the masking and the bounds, are kept).  Also: the header declares the new entry points and the library exports them."""
import math
import os

import pytest
import torch

from tests import entropy_ref as ER
from tests import grpo_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SHAPES = [(min(R, 24), V, H) for R, V, H, _ in ER.SHAPES]
_cache = {}


def _case(shape):
    if shape not in _cache:
        R, V, H = shape
        c = ER.make_case(R, V, H, seed=R + V + H)
        c["ref"] = ER.forward_reference(c["hg"], c["w"], c["tgt"])
        g = torch.Generator().manual_seed(7)
        c["dlogp"], c["dent"] = torch.randn(R, generator=g), torch.randn(R, generator=g)
        _cache[shape] = c
    return _cache[shape]


def test_exports_and_header():
    from vlrlhf import _hip
    l = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "vlr.h")).read()
    for name in ("vlr_lmhead_logps_entropy_fwd", "vlr_lmhead_logps_entropy_bwd", "vlr_lmhead_entropy_workspace_bytes", "vlr_logp_ent_rows",
                 "vlr_dlogits_ent_rows", "vlr_grpo_loss_ent"):
        assert name + "(" in hdr and hasattr(l, name) and name in _hip.exported_symbols(), name
    assert _hip.helper("vlr_abi_version") == 9               # additive entry points: no caller breaks
    R, V = 2100, 8200
    parts = ((V + 255) // 256) * 4
    assert int(l.vlr_lmhead_entropy_workspace_bytes(R, V)) == (R * parts * 3 + 2 * R) * 4
    assert int(l.vlr_lmhead_workspace_bytes(R, V)) == (R * parts * 2 + 2 * R) * 4       # the existing one is untouched
    assert l.vlr_lmhead_logps_entropy_fwd(None, None, None, None, None, None, None, None, 8, 8, 8, None) == 1
    assert b"vlr_lmhead_logps_entropy_fwd: null operand" in l.vlr_last_error()
    assert l.vlr_lmhead_logps_entropy_bwd(None, None, None, None, None, None, None, None, None, None, 8, 8, 8, None) == 1
    assert b"vlr_lmhead_logps_entropy_bwd: null operand" in l.vlr_last_error()
    assert l.vlr_grpo_loss_ent(None, None, None, None, None, 4, 2, 0.2, 0.2, 0.0, 0, 0, 1.0, None, None, 0.0, None, None, None, None) == 1
    assert b"vlr_grpo_loss_ent: null operand" in l.vlr_last_error()


@pytest.mark.parametrize("shape", HOST_SHAPES)
def test_planted_rows_and_reference(shape):
    R, V, H = shape
    c = _case(shape)
    ref = c["ref"]
    for r, kind in enumerate(c["kinds"]):
        if kind == "zero":
            assert abs(float(ref["H"][r]) - math.log(V)) < 1e-12 and float(ref["ez"][r]) == 0.0
        elif kind.startswith("dom@"):
            z = c["hg"][r].double() @ c["w"].double().t()
            assert int(z.argmax()) == int(c["tgt"][r]) == int(kind[4:])
            assert float(z.max() - z.topk(2).values[1]) > 100 and float(ref["H"][r]) < 1e-40
        elif kind == "tie":
            z = c["hg"][r].double() @ c["w"].double().t()
            top = (z == z.max()).nonzero().flatten().tolist()
            assert len(top) == 2 and (V <= 256 or top[0] // 256 != top[1] // 256)
    if R >= 8:
        assert {"zero", "tie"} <= set(c["kinds"]) and sum(k.startswith("dom@") for k in c["kinds"]) == len(ER.dominant_columns(V))
    # the bounds are small against what they guard: a random row's entropy is known to better than a percent of a nat
    rnd = [r for r, k in enumerate(c["kinds"]) if k == "random"]
    assert float(ref["b_H"][rnd].max()) < 1e-2


@pytest.mark.parametrize("shape", HOST_SHAPES)
def test_checker_accepts_the_replay_and_flags_forward_faults(shape):
    R, V, H = shape
    c = _case(shape)
    tok, lse, Hh = ER.replay_forward(c["hg"], c["w"], c["tgt"])
    fails, worst = ER.check_entropy(Hh, c["ref"], V)
    assert fails == [] and worst <= 1.0, fails
    assert bool(((lse.double() - c["ref"]["lse"]).abs() <= c["ref"]["b_lse"]).all())
    assert bool(((tok.double() - c["ref"]["tok"]).abs() <= c["ref"]["b_tok"]).all())
    for fault in ER.FWD_FAULTS:
        if fault in ("skip_last_tile", "unmasked_last_tile") and V % 256 == 0:
            continue                                           # no partial column tile in this shape
        if fault == "skip_last_tile" and V < 256:
            continue                                           # the partial tile is the only one
        if fault in ("drop_shift", "own_max") and V <= 64:
            continue                                           # one part: nothing to shift
        _, _, bad = ER.replay_forward(c["hg"], c["w"], c["tgt"], fault=fault)
        fails, _ = ER.check_entropy(bad, c["ref"], V)
        assert fails, f"{fault} passed the checker on {shape}"


@pytest.mark.parametrize("shape", HOST_SHAPES)
def test_checker_accepts_the_replay_and_flags_backward_faults(shape):
    R, V, H = shape
    c = _case(shape)
    _, lse, Hh = ER.replay_forward(c["hg"], c["w"], c["tgt"])
    zero = torch.zeros(R)
    for dlogp, dent in ((c["dlogp"], c["dent"]), (zero, c["dent"]), (c["dlogp"], zero)):
        dl = ER.replay_backward(c["hg"], c["w"], c["tgt"], lse, Hh, dlogp, dent)
        fails, worst = ER.check_dlogits(dl, c["hg"], c["w"], c["tgt"], c["ref"], dlogp, dent)
        assert fails == [] and worst <= 1.0, fails
    for fault in ER.BWD_FAULTS:
        dl = ER.replay_backward(c["hg"], c["w"], c["tgt"], lse, Hh, c["dlogp"], c["dent"], fault=fault)
        fails, _ = ER.check_dlogits(dl, c["hg"], c["w"], c["tgt"], c["ref"], c["dlogp"], c["dent"])
        assert fails, f"{fault} passed the checker on {shape}"


@pytest.mark.parametrize("lt", sorted(GR.LOSS_TYPES))
def test_grpo_ent_checker(lt):
    lengths = [40, 1, 70, 9, 30, 2, 64, 65, 3, 17, 128, 5, 33, 1, 90, 7, 66]
    logp, old, ref, adv, so = GR.branch_inputs(lengths, [1.5, -0.75, -1.25, 0.0, 2.0], 0.2, 0.28, seed=3)
    R = sum(lengths)
    g = torch.Generator().manual_seed(4)
    Hh = torch.rand(R, generator=g) * 3
    keep = torch.rand(R, generator=g) < 0.5
    args = (logp, old, ref, adv, so, 0.2, 0.28, 0.04, lt, 48, 0.5, Hh, keep, 0.01)
    dlogp, dent, stats = ER.replay_grpo_ent(*args)
    fails, worst = ER.check_grpo_ent(dlogp, dent, stats, *args)
    assert fails == [] and worst <= 1.0, fails
    assert abs(float(stats[9]) - float(keep.float().mean())) < 1e-6 and abs(float(stats[8]) - float(Hh.mean())) < 1e-5
    dlogp, dent, stats = ER.replay_grpo_ent(*args, fault="keep_ignored")
    fails, _ = ER.check_grpo_ent(dlogp, dent, stats, *args)
    assert any("masked token" in f for f in fails), fails
    # the mask and the bonus are in the loss: without them it is vlr_grpo_loss's
    plain = ER.grpo_ent_loss(logp.double(), old.double(), ref.double(), adv.double(), so, 0.2, 0.28, 0.04, lt, 48, 0.5, None, None, 0.0)
    want = GR.loss(logp.double(), old.double(), ref.double(), adv.double(), so, 0.2, 0.28, 0.04, lt, 48, 0.5)
    assert float(plain[0]) == float(want[0]) and all(plain[1][k] == want[1][k] for k in GR.STAT_NAMES)
