"""The row-compact reference pass (engine.forward_hidden(prefix_dedup_rows=True), vlr_decoder_layer_fwd_compact): each DPO pair's shared
prompt rows are computed once.  Against the golden vectors, the fp32 oracle and the dense pass of the same binary (engine.prefix_dedup =
False), on the toy LLaVA fixture and - one layer through the C ABI - at the 7B widths.  Needs a real MI355X:  pytest -m gpu"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import llava_dpo_oracle as O  # noqa: E402  (checker only)
from tests.golden_util import load_case, t  # noqa: E402
from tests.test_hip_e2e import TOL_LOGPS_FP32, TOL_LOSS_FP32, build, make_trainer, relmax  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return torch.device("cuda")


def _ref_logps(tr, batch, eng, on):
    eng.prefix_dedup, eng.prefix_dedup_min_share = on, 0.0
    n0 = eng.prefix_dedup_passes
    rc, rr = tr._reference_logps(dict(batch))          # a fresh dict: the per-batch cache of the trainer is rebuilt
    torch.cuda.synchronize()
    return torch.cat([rc, rr]).float().cpu(), eng.prefix_dedup_passes - n0


def test_reference_logps_match_golden_and_dense(gpu):
    """the trainer's reference forward on the golden fixture: switch on against the golden log-probs and against the switch-off run, both
    within the bound the dense path is held to; the engine's counter says which path ran"""
    z, cfg, W, W_ref, batch, rows = load_case("llava_hipsmall")
    model, ref = build(cfg, W, W_ref)
    tr = make_trainer(model, ref, cfg)
    eng = model.engine
    assert eng.prefix_dedup and eng.prefix_dedup_min_share == 1.0 / 8           # the defaults
    on, ran_on = _ref_logps(tr, batch, eng, True)
    off, ran_off = _ref_logps(tr, batch, eng, False)
    assert ran_on == 1 and ran_off == 0
    d = eng.last_prefix_dedup
    B = batch["chosen_input_ids"].shape[0]
    assert len(d["P"]) == B and min(d["P"]) >= batch["prompt_input_ids"].shape[1] and d["Mc"] == d["M"] - sum(d["P"]), d
    gold = t(z, "ref_logps")
    print(f"ref log-probs: on - golden {float((on - gold).abs().max()):.4f}, off - golden {float((off - gold).abs().max()):.4f}, "
          f"on - off {float((on - off).abs().max()):.4f}; P {d['P']} rows {d['Mc']} of {d['M']}")
    assert float((on - gold).abs().max()) < TOL_LOGPS_FP32
    assert float((on - off).abs().max()) < TOL_LOGPS_FP32
    # no other caller gets the compact pass: a plain no-grad forward of the same model and batch stays dense
    n0 = eng.prefix_dedup_passes
    eng.prefix_dedup = True
    with torch.no_grad():
        tr.concatenated_forward(ref, dict(batch))
    assert eng.prefix_dedup_passes == n0
    # ... and below the floor the reference pass is the dense one, bit for bit
    eng.prefix_dedup_min_share = 0.9
    rc, rr = tr._reference_logps(dict(batch))
    assert eng.prefix_dedup_passes == n0
    assert torch.equal(torch.cat([rc, rr]).float().cpu(), off)


def _edited_batch(cfg):
    """three ragged pairs: pair 0 - the rejected prompt differs at token 1; pair 1 - rejected == chosen; pair 2 - the shared rows end off
    every 8-row boundary (the rejected prompt differs three tokens before its end)"""
    lp = 24
    batch = O.synthetic_batch(3, 48, cfg["image_token"], 170, cfg["image_size"], seed=11, ragged=True)
    n = max(batch["chosen_input_ids"].shape[1], batch["rejected_input_ids"].shape[1])
    for side in ("chosen", "rejected"):
        for field, pad in (("input_ids", 0), ("attention_mask", 0), ("labels", -100)):
            v = batch[f"{side}_{field}"]
            batch[f"{side}_{field}"] = torch.cat([v, torch.full((v.shape[0], n - v.shape[1]), pad, dtype=v.dtype)], dim=1)
    batch["rejected_input_ids"][0, 1] = 171
    for field in ("input_ids", "attention_mask", "labels"):
        batch[f"rejected_{field}"][1] = batch[f"chosen_{field}"][1]
    batch["rejected_input_ids"][2, lp - 3] = 172
    batch["img_path"] = ["synthetic"] * 3
    return batch, lp


def test_hidden_states_edited_prefixes(gpu):
    z, cfg, W, W_ref, _, _ = load_case("llava_hipsmall")
    model, ref = build(cfg, W, W_ref)
    tr = make_trainer(model, ref, cfg)
    eng = model.engine
    batch, lp = _edited_batch(cfg)
    B = 3
    Pimg = (cfg["image_size"] // cfg["patch_size"]) ** 2
    outs = {}
    for on in (True, False):
        eng.prefix_dedup, eng.prefix_dedup_min_share = on, 0.0
        cb = tr.concatenated_inputs(dict(batch), device=gpu)
        n0 = eng.prefix_dedup_passes
        with torch.no_grad(), ref.reference_pass():
            out = ref(input_ids=cb["concatenated_input_ids"], attention_mask=cb["concatenated_attention_mask"],
                      labels=cb["concatenated_labels"], use_cache=False, **cb["concatenated_img_input_dict"])
        assert eng.prefix_dedup_passes - n0 == int(on)
        c = out.logits.c
        S = c["S"]
        assert tuple(c["hidden"].shape) == (2 * B * S, cfg["hidden"]) and c["M"] == 2 * B * S
        outs[on] = dict(hidden=c["hidden"].float().cpu().reshape(2 * B, S, -1), logits=out.logits.materialize().float().cpu(),
                        mean=float(out.logits[:B].mean()), mask=c["mask"].cpu().reshape(2 * B, S), pos=c["pos"].cpu().reshape(2 * B, S), S=S)
    S = outs[True]["S"]
    P = eng.last_prefix_dedup["P"]
    assert P == [1, S, lp - 3 + Pimg - 1], P
    assert P[2] % 8 != 0
    assert torch.equal(outs[True]["mask"], outs[False]["mask"]) and torch.equal(outs[True]["pos"], outs[False]["pos"])
    # the oracle in fp32 on the reference weights (bf16-representable, as the engine stores them)
    Wf = {k: v.bfloat16().float() for k, v in W_ref.items()}
    cbo = O.concatenated_inputs(batch)
    with torch.no_grad():
        hid32, _, aux = O.llava_forward(Wf, cfg, cbo["concatenated_input_ids"], cbo["concatenated_attention_mask"], cbo["concatenated_labels"],
                                        cbo["concatenated_img_input_dict"]["pixel_values"], False, return_hidden=True)
        log32 = O.lm_logits(hid32, Wf)
    valid = aux["mask"].bool()
    assert torch.equal(valid, outs[True]["mask"].bool())
    for on in (True, False):
        eh, el = relmax(outs[on]["hidden"][valid], hid32[valid]), relmax(outs[on]["logits"][valid], log32[valid])
        print(f"prefix_dedup {on}: hidden relmax {eh:.3e}, logits relmax {el:.3e} against the fp32 oracle")
        assert eh < 4e-2 and el < 4e-2
        assert tuple(outs[on]["logits"].shape) == tuple(log32.shape)
        assert abs(outs[on]["mean"] - float(log32[:B].mean())) < 2e-2 * float(log32.abs().mean()) + 1e-3
    hid = outs[True]["hidden"]
    for i in range(B):                        # the dropped rows are copies of their chosen twins
        assert torch.equal(hid[B + i, :P[i]], hid[i, :P[i]])


def test_side_stream_step(gpu):
    """the trainer's step with the reference forward on the side stream: golden loss with the switch on and off, and two runs with the
    switch on agree bit for bit (loss and every gradient)"""
    z, cfg, W, W_ref, batch, rows = load_case("llava_hipsmall")
    exp = float(z["loss_mean_sigmoid"])
    outs = []
    for on in (True, True, False):
        model, ref = build(cfg, W, W_ref)
        tr = make_trainer(model, ref, cfg)
        assert tr.ref_on_side_stream
        eng = model.engine
        eng.prefix_dedup, eng.prefix_dedup_min_share = on, 0.0
        loss = tr.training_step(model, dict(batch))
        torch.cuda.synchronize()
        assert eng.prefix_dedup_passes == int(on)
        print(f"prefix_dedup {on}: loss {float(loss):.6f} golden {exp:.6f}")
        assert abs(float(loss) - exp) < TOL_LOSS_FP32, (on, float(loss), exp)
        outs.append((float(loss), eng.grads.clone()))
    assert outs[0][0] == outs[1][0]
    assert torch.equal(outs[0][1], outs[1][1])


def _rnd(*shape, scale=1.0, seed=0, dtype=torch.bfloat16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(dtype)


def _acts(hip, rows, B, S, H, I, nh, Nq, Nqkv):
    Sp = (S + 63) // 64 * 64
    nan = lambda *s, dt=torch.bfloat16: torch.full(s, float("nan"), dtype=dt, device=DEV)      # noqa: E731
    a = dict(xn1=nan(rows, H), rstd1=nan(rows, dt=torch.float32), qkv=nan(rows, Nqkv), attn=nan(rows, Nq),
             lse=nan(B, nh, Sp, dt=torch.float32), x_mid=nan(rows, H, dt=torch.float32), xn2=nan(rows, H), rstd2=nan(rows, dt=torch.float32),
             gu=nan(rows, 2 * I), act=nan(rows, I), x_out=nan(rows, H, dt=torch.float32))
    a["struct"] = hip.LayerActs(*(a[n].data_ptr() for n in ("xn1", "rstd1", "qkv", "attn", "lse", "x_mid", "xn2", "rstd2", "gu", "act", "x_out")))
    return a


@pytest.mark.parametrize("pairs", [2, 4])
def test_compact_layer_true_widths_matches_dense(gpu, pairs):
    """ONE layer at the 7B widths through the C ABI: 2 pairs of S = 1599 with 1087 shared rows (the benchmark's geometry), M = 6396 dense and
    4222 compact rows - the persistent 256 x 256 kernel and its peeled tail at a row count the dense pass never has; and the benchmark's
    own 4 pairs (12 792 / 8444 rows), where the dense residual projections peel their last 504 rows to the split-K kernel and the compact
    ones would peel 252 of their own accord.  The peeled rows lie inside the kept tail (512 rows), so every row runs in the kernel the
    dense pass runs it in: the kept rows are BIT-IDENTICAL to the dense layer's.  With the tail withheld (tail_rows = 0) the launches
    split on their own row count and the rows answer to the bound alone.
    Bound: tests/test_hip_true_width.py judges whole models on their log-probs and has no row-wise figure; the row-wise statement here
    is the one tests/test_hip_decode_kernels.py::test_decoder_layer_decode_matches_prefill makes for two routes through this same layer
    at these widths - the layer's update x_out - x_in within 2e-2 of its largest magnitude (bf16 rounding of q|k|v, attention output and
    silu(g) * u, whose fp32 sums the two routes form in a different order).  Prints the share of bit-identical rows."""
    from vlrlhf import _hip as hip
    from vlrlhf import prefix_dedup as PD
    H, I, nh, hd, max_pos = 4096, 11008, 32, 128, 4096
    Nq = nh * hd
    N = 3 * Nq
    S, P = 1599, 1087
    Bn = 2 * pairs
    M = Bn * S
    cos = torch.empty(max_pos, hd // 2, dtype=torch.float32, device=DEV)
    sin = torch.empty_like(cos)
    hip.call("vlr_rope_table", cos, sin, max_pos, hd, 10000.0)
    cfg = hip.LlamaCfg(H, I, nh, hd, 1e-5, max_pos, cos.data_ptr(), sin.data_ptr(), nh, 1)
    sc = 1.0 / math.sqrt(H)
    W = dict(ln1=(1 + 0.1 * _rnd(H, seed=20).float()).bfloat16(), wqkv=_rnd(N, H, scale=sc, seed=21), wo=_rnd(H, Nq, scale=sc, seed=22),
             ln2=(1 + 0.1 * _rnd(H, seed=23).float()).bfloat16(), wgu=_rnd(2 * I, H, scale=sc, seed=24), wdown=_rnd(H, I, scale=1 / math.sqrt(I), seed=25))
    lw = hip.LayerWeights(*(W[k].data_ptr() for k in ("ln1", "wqkv", "wo", "ln2", "wgu", "wdown")), None)
    x = _rnd(Bn, S, H, seed=26, dtype=torch.float32)
    x[pairs:, :P] = x[:pairs, :P]                                   # the shared prompt
    x = x.reshape(M, H).contiguous()
    km = torch.ones(Bn, S, dtype=torch.int32, device=DEV)
    pos = torch.arange(S, dtype=torch.int32, device=DEV).repeat(Bn, 1).contiguous()
    rows, dsrc = PD.build_row_maps([P] * pairs, S)
    Mc = rows.numel()
    assert (M, Mc) == {2: (6396, 4222), 4: (12792, 8444)}[pairs]
    assert hip.helper("vlr_gemm_peel_rows", M, H) == {2: 0, 4: 504}[pairs] and hip.helper("vlr_gemm_peel_rows", Mc, H) == {2: 0, 4: 252}[pairs]
    rows, dsrc = rows.to(DEV), dsrc.to(DEV)
    ad = _acts(hip, M, Bn, S, H, I, nh, Nq, N)
    hip.call("vlr_decoder_layer_fwd_ex", cfg, lw, ad["struct"], x, pos, km, Bn, S, 0)
    ac = _acts(hip, Mc, Bn, S, H, I, nh, Nq, N)
    xc = x[rows.long()].contiguous()
    pc = pos.reshape(-1)[rows.long()].contiguous()
    qkv_d = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    attn_d = torch.full((M, Nq), float("nan"), dtype=torch.bfloat16, device=DEV)
    dense = ad["x_out"][rows.long()]
    for tail in (S - P, 0):
        ac["x_out"].fill_(float("nan"))
        hip.call("vlr_decoder_layer_fwd_compact", cfg, lw, ac["struct"], xc, pc, dsrc, rows, Mc, tail, qkv_d, attn_d, km, Bn, S)
        torch.cuda.synchronize()
        got = ac["x_out"]
        assert torch.isfinite(got).all() and torch.isfinite(dense).all()
        same = float((got == dense).all(dim=1).float().mean())
        e = relmax(got - xc, dense - xc)
        print(f"compact layer at 7B widths, {pairs} pairs, tail_rows {tail}: update relmax {e:.3e} against the dense layer; "
              f"{100 * same:.2f} % of the {Mc} rows bit-identical")
        assert e <= 2e-2
        if tail:
            assert torch.equal(got, dense)
    with pytest.raises(ValueError, match="compact rows"):
        hip.call("vlr_decoder_layer_fwd_compact", cfg, lw, ac["struct"], xc, pc, dsrc, rows, M + 1, 0, qkv_d, attn_d, km, Bn, S)
    with pytest.raises(ValueError, match="tail rows"):
        hip.call("vlr_decoder_layer_fwd_compact", cfg, lw, ac["struct"], xc, pc, dsrc, rows, Mc, Mc + 1, qkv_d, attn_d, km, Bn, S)
