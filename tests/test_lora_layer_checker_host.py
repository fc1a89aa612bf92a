"""The checker of tests/lora_layer_ref.py on the CPU (no GPU, no marker): the unfaulted bf16 replay of the LoRA decoder-layer passes sits
under a quarter of the bounds tests/test_hip_lora_layer.py applies to the kernels, in every case and tensor; every planted wiring fault
exceeds those bounds in every case that takes the faulted code (the table is printed); the case table holds both sides of every branch
of the drivers for each family; the restated layer agrees with the oracle's llama_hidden where that fits; and the argument rules of
lora_check / lora2_check (csrc/layers.cpp) refuse before any launch."""
import ctypes as C
import functools

import pytest
import torch

from oracle import llava_dpo_oracle as O
from tests import lora_layer_ref as R

# a chain of at most 16 bf16 stores lies between an operand and any compared tensor (xn, u, qkv, attn, x_mid, xn2, gu, act, x_out on
# the way down; v, dact, dgu, dxn twice, dx_mid, dattn twice, dqkv twice, the output on the way up, never all on one path), each worth
# at most 2^-9 of the element it rounds: the replay's err stays under 16 * 2^-9
REPLAY_CEILING = 16 * 2.0 ** -9


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = R.BY_NAME[name]
    inp = R.make(c)
    return c, inp, R.measure(c, inp, inp["ref"], R.replay(c, inp))


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_unfaulted_replay_sits_under_a_quarter_of_the_bounds(name):
    c, inp, meas = _inputs(name)
    assert set(meas) == set(R.tensors(c)) and {"x_out", "u", "dx_in", "dA_qkv", "dB_gu"} <= set(meas)
    for n, (err, scale) in meas.items():
        be, bc = R.bounds(err, scale)
        assert err <= be / R.MARGIN and abs(scale - 1) <= bc / R.MARGIN, (n, err, scale)          # by construction: bound = 4 x replay (+ 2^-9)
        assert err < REPLAY_CEILING and abs(scale - 1) < R.C_FLOOR, (n, err, scale)
    rat = R.ratios(meas, meas)
    assert all(a <= 0.25 and b <= 0.25 for a, b in rat.values()), rat
    ref = inp["ref"]
    if c.rowmask == "zero":                                       # no image row: the row-restricted adapter's products are exactly zero
        R_ = c.r + (c.r_p if c.family == "lora2" else 0)
        u = ref["u"].view(c.M, 7, R_)[:, :, (c.r if c.family == "lora2" else 0):]
        assert float(u.nan_to_num().abs().max()) == 0.0
        if c.family == "lora_ex":
            assert all(float(ref[n].abs().max()) == 0.0 for n in R.LORA_GRADS) and all(meas[n] == (0.0, 1.0) for n in R.LORA_GRADS)
    else:
        assert all(float(ref[n].abs().max()) > 0 for n in R.tensors(c) if n != "u")
    assert float(ref["dx_in"][~inp["valid"]].abs().max()) == 0.0   # dy is zero on the padded rows and nothing attends to them


def test_every_planted_fault_exceeds_the_bounds():
    table = {}
    for f in R.FAULTS:
        for case in R.CASES:
            if not R.exercises(case, f):
                continue
            c, inp, meas = _inputs(case.name)
            rat = R.ratios(R.measure(c, inp, inp["ref"], R.replay(c, inp, f)), meas)
            n, (re_, rc) = max(rat.items(), key=lambda kv: max(kv[1]))
            table.setdefault(f, []).append((c.name, n, re_, rc))
    print("\nfault -> cases that take the faulted code: worst tensor, err / bound, |c - 1| / bound")
    for f in R.FAULTS:
        print(f"  {f}")
        for name, n, re_, rc in table.get(f, []):
            print(f"      {name:48s} {n:8s} {re_:9.2f} {rc:9.2f}  {'caught' if max(re_, rc) > 1 else 'MISSED'}")
    for f in R.FAULTS:
        assert table.get(f), f"no case exercises {f}"
        for fam in ("lora", "lora_ex", "lora2"):                  # a fault a family can take is exercised in that family
            can = fam == "lora2" if f.startswith("plora_") else fam == "lora_ex" if f == "ln_grad_without_adapter_dx" else \
                fam != "lora" if f in ("mask_compact_index", "text_rows_leak", "tile_skipped_with_marked_last_row") else True
            assert not can or any(R.BY_NAME[name].family == fam for name, *_ in table[f]), (f, fam)
        assert all(max(re_, rc) > 1 for _, _, re_, rc in table[f]), (f, table[f])


def test_case_table_covers_every_branch():
    for fam, need in R.REQUIRED.items():
        have = set().union(*(R.branches(c) for c in R.CASES if c.family == fam))
        assert need <= have, (fam, sorted(need - have))
    assert {c.M for c in R.CASES} == {140, 320, 768} and {c.r for c in R.CASES} == {8, 64}
    assert {c.r_p for c in R.CASES if c.family == "lora2"} == {8, 256} and {c.kv_heads for c in R.CASES} == {1, 2}
    assert all(c.hidden == 256 and c.inter == 384 and c.heads * R.HEAD_DIM == c.hidden for c in R.CASES)
    assert any(c.bias for c in R.CASES) and {c.dropout for c in R.CASES} == {0.0, 0.25}
    for c in R.CASES:
        m = R.row_mask(c.rowmask, c.B, c.S)
        if c.rowmask == "edge":
            assert m.nonzero().flatten().tolist() == [255, 256, c.M - 1]
        if c.rowmask == "one_tile_empty":
            assert c.M == 768 and not m[256:512].any() and m[:256].any() and m[512:].any() and m[255] and m[512]
        if c.rowmask == "ragged":
            runs = (m.view(c.B, c.S).int().diff(dim=1) == 1).sum(1) + m.view(c.B, c.S)[:, 0].int()
            assert runs.tolist() == [2] * c.B
        if c.rowmask == "zero":
            assert not m.any()
        if c.mask_bits or c.mask_bits_p:
            assert (c.M * c.hidden) % 32 == 0 and (c.M * c.inter) % 32 == 0


def test_restated_layer_agrees_with_the_oracle_where_it_fits():
    """peft LoRA on q, k, v, o, gate, up, down with dropout, multi-head attention, no bias, no row mask: llama_hidden (layers = 1,
    collect, lora=) computes the same layer; in fp32 the two agree to fp32 rounding, masks and RoPE tables included"""
    c = R.BY_NAME["lora_m140_r8_hash"]
    inp = R.make(c)
    a = inp["sets"][0]
    p = "language_model.model.layers.0."
    H, I = c.hidden, c.inter
    W = {p + "input_layernorm.weight": inp["ln1"], p + "post_attention_layernorm.weight": inp["ln2"],
         p + "self_attn.o_proj.weight": inp["wo"], p + "mlp.down_proj.weight": inp["wdown"],
         p + "mlp.gate_proj.weight": inp["wgu"][:I], p + "mlp.up_proj.weight": inp["wgu"][I:], "language_model.model.norm.weight": torch.ones(H)}
    for i, n in enumerate("qkv"):
        W[p + f"self_attn.{n}_proj.weight"] = inp["wqkv"][i * H:(i + 1) * H]
    W = {k: v.float() for k, v in W.items()}
    LW = {}
    for t, (grp, i, rows) in zip(O.LORA_TARGETS, (("qkv", 0, (0, H)), ("qkv", 1, (H, 2 * H)), ("qkv", 2, (2 * H, 3 * H)), ("o", 0, (0, H)),
                                                  ("gu", 0, (0, I)), ("gu", 1, (I, 2 * I)), ("down", 0, (0, H)))):
        na, nb = O.lora_names(0, t)
        LW[na], LW[nb] = a["A_" + grp][i * c.r:(i + 1) * c.r].float(), a["B_" + grp][rows[0]:rows[1]].float()
    lora = dict(W=LW, scale=a["scale"], dropout=a["p"], seed=a["seed"], r=c.r)
    col = []
    cfg = dict(hidden=H, inter=I, layers=1, heads=c.heads, vocab=8, rms_eps=R.EPS)
    O.llama_hidden(inp["x_in"].float().view(c.B, c.S, H), inp["key_mask"], inp["pos"], W, cfg, collect=col, lora=lora)
    mine = R.forward(c, inp, R.F32, lambda t: t)["x_out"]
    assert float((mine - col[0].view(c.M, H)).abs().max()) < 1e-4 * float(mine.abs().max())
    assert float((R.forward(c, inp, R.F64, lambda t: t)["x_out"] - inp["ref"]["x_out"]).abs().max()) == 0.0


def test_packed_mask_offsets_fit_the_buffer():
    from vlrlhf import _hip
    l = _hip.lib()
    for c in R.CASES:
        if not (c.mask_bits or c.mask_bits_p):
            continue
        M, H, I = c.M, c.hidden, c.inter
        assert [R.bits_offset(c, t) for t in (0, 3, 6)] == [0, 3 * M * H // 8, 6 * M * H // 8]
        assert R.bits_offset(c, 6) + M * I // 8 <= int(l.vlr_lora_mask_bytes(H, I, M))
    c = R.BY_NAME["lora_m140_r64_bits_gqa_fusedqkv"]
    a = R.make(c)["sets"][0]
    bits, keep = R.packed_bits(a, 6, c.M, c.inter), O.dropout_mask(a["seed"] + 6, c.M * c.inter, a["p"])
    for e in (0, 1, 7, 8, 9, c.M * c.inter - 1):                  # include/vlr.h: bit e of byte i = element 8 i + e
        assert (int(bits[e // 8]) >> (e % 8)) & 1 == int(keep[e])


# ---------------------------------------------------------------------------------------------------- argument rules
FAKE = 1 << 20          # a non-null pointer that is never dereferenced: every call below is refused by the argument checks


def _structs(**kw):
    from vlrlhf import _hip as HH
    cfg = HH.LlamaCfg(256, 384, 2, 128, 1e-5, 512, FAKE, FAKE, 2, 0)
    w = HH.LayerWeights(*([FAKE] * 6), None)
    a = HH.LayerActs(*([FAKE] * 11))
    ws = HH.LayerBwdWs(*([FAKE] * 7))
    lg = HH.LoraGrads(*([FAKE] * 8))
    return HH, cfg, w, a, ws, lg


def _lw(HH, r=8, dropout=0.0, qkv_targets=3, a_down=FAKE, b_down=FAKE):
    return HH.LoraWeights(r, 2.0, dropout, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, a_down, b_down, qkv_targets, None)


def _refused(l, rc, text):
    assert rc == 1 and text.encode() in l.vlr_last_error(), (rc, l.vlr_last_error())


@pytest.mark.parametrize("kw,text", [
    (dict(r=12), "LoRA rank must be a positive multiple of 8, got 12"),
    (dict(r=0), "LoRA rank must be a positive multiple of 8, got 0"),
    (dict(dropout=1.0), "lora_dropout must be in [0,1), got 1"),
    (dict(dropout=-0.25), "lora_dropout must be in [0,1), got -0.25"),
    (dict(qkv_targets=2), "qkv_targets must be 1 or 3, got 2"),
    (dict(b_down=None), "null adapter pointer"),
    (dict(a_down=None), "null adapter pointer"),
])
def test_lora_check_refuses_before_any_launch(kw, text):
    HH, cfg, w, a, ws, lg = _structs()
    l = HH.lib()
    lw = _lw(HH, **kw)
    r = C.byref
    _refused(l, l.vlr_decoder_layer_fwd_lora(r(cfg), r(w), r(lw), r(a), FAKE, None, 1, FAKE, FAKE, None, 2, 8, None), text)
    _refused(l, l.vlr_decoder_layer_fwd_lora_ex(r(cfg), r(w), r(lw), r(a), FAKE, None, 1, None, FAKE, FAKE, None, 2, 8, None), text)
    _refused(l, l.vlr_decoder_layer_bwd_lora(r(cfg), r(w), r(lw), r(lg), 0, r(a), FAKE, r(ws), FAKE, FAKE, 1, FAKE, FAKE, FAKE, FAKE, None,
                                             2, 8, None), text)
    _refused(l, l.vlr_decoder_layer_bwd_lora_ex(r(cfg), r(w), None, r(lw), r(lg), 0, r(a), FAKE, r(ws), FAKE, FAKE, 1, None, FAKE, FAKE, FAKE,
                                                FAKE, None, 2, 8, None), text)
    good = _lw(HH)
    bc = HH.LoraBcomb(FAKE, FAKE, FAKE, FAKE)
    for lw2, pw2 in ((lw, good), (good, lw)):                     # either adapter of the two-adapter passes
        if "null adapter pointer" in text and lw2 is good:
            continue                                              # (a half-set down pair on one side alone: the rule below, tested there)
        _refused(l, l.vlr_decoder_layer_fwd_lora2(r(cfg), r(w), r(lw2), r(pw2), r(bc), r(a), FAKE, 1, 2, None, FAKE, FAKE, None, 2, 8, None), text)
        _refused(l, l.vlr_decoder_layer_bwd_lora2(r(cfg), r(w), r(lw2), r(lg), r(pw2), r(bc), 0, r(a), FAKE, r(ws), FAKE, 1, 2, None, FAKE,
                                                  FAKE, FAKE, FAKE, None, 2, 8, None), text)


def test_lora2_check_refuses_before_any_launch():
    HH, cfg, w, a, ws, lg = _structs()
    l = HH.lib()
    r = C.byref

    def both(lw, pw, bc, text):
        bcp = None if bc is None else r(bc)
        _refused(l, l.vlr_decoder_layer_fwd_lora2(r(cfg), r(w), r(lw), r(pw), bcp, r(a), FAKE, 1, 2, None, FAKE, FAKE, None, 2, 8, None), text)
        _refused(l, l.vlr_decoder_layer_bwd_lora2(r(cfg), r(w), r(lw), r(lg), r(pw), bcp, 0, r(a), FAKE, r(ws), FAKE, 1, 2, None, FAKE, FAKE,
                                                  FAKE, FAKE, None, 2, 8, None), text)

    full = HH.LoraBcomb(FAKE, FAKE, FAKE, FAKE)
    both(_lw(HH), _lw(HH, r=256), None, "null concatenated B")
    both(_lw(HH), _lw(HH, r=256), HH.LoraBcomb(FAKE, None, FAKE, FAKE), "null concatenated B")
    both(_lw(HH, qkv_targets=1), _lw(HH, qkv_targets=3), full, "the two adapters must split the qkv projection the same way")
    both(_lw(HH, qkv_targets=0), _lw(HH, qkv_targets=1), full, "the two adapters must split the qkv projection the same way")
    both(_lw(HH), _lw(HH, a_down=None, b_down=None), full, "down-projection adapters must be both present or both absent")
    both(_lw(HH, a_down=None, b_down=None), _lw(HH), full, "down-projection adapters must be both present or both absent")
    both(_lw(HH), _lw(HH), HH.LoraBcomb(FAKE, FAKE, FAKE, None), "down-projection adapters must be both present or both absent")
