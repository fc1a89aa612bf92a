"""GPTQ int4 base weights (q_lora) on the MI355X: the dequantising transpose, the packed skinny GEMM and the engine over a packed
base.  The acceptance criterion of the training path is bit-identity with a bf16 run on the host-dequantised weights; the decode path
adds the same bf16 products in another order.  Outputs are NaN-poisoned before every call.  Needs a real MI355X:  pytest -m gpu"""
import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gptq_ref as R  # noqa: E402
from tests.golden_util import load_case  # noqa: E402

DEV = "cuda"
PEFT = dict(r=8, lora_alpha=16, lora_dropout=0.05, target_modules="auto", bias="none", seed=5)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return _hip


def relerr(a, b):
    a, b = a.float(), b.float()
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-12)


def check(a, b, tol, what=""):
    e = relerr(a, b)
    print(f"{what}: rel err {e:.3e} (bound {tol:.1e})")
    assert math.isfinite(e) and e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"


def nan_like(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


_CASES = {}


def packed_case(K, N, g):
    """random q / zeros / scales of one linear, packed, on the device, with the reference W (computed once per shape and shared).
    Zeros cover 1 .. 16 (every group row of the first 16 columns walks through them); column 1 is all-15 nibbles, column 2 all-0."""
    key = (K, N, g)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(K * 31 + N * 7 + (g % 1000))
        G = K // R.group(K, g)
        q = torch.randint(0, 16, (K, N), generator=gen, dtype=torch.int32)
        q[:, 1], q[:, 2] = 15, 0
        zero = torch.randint(1, 17, (G, N), generator=gen, dtype=torch.int32)
        zero[:, :16] = (torch.arange(16)[None, :] + torch.arange(G)[:, None]) % 16 + 1
        scales = (torch.rand(G, N, generator=gen) * 0.02 + 0.002).half()
        t = {k: v.to(DEV) for k, v in R.pack(q, zero, scales, g).items()}
        t["W"] = R.dequant(t["qweight"], t["qzeros"], t["scales"], g)
        assert set(zero[:, :16].reshape(-1).tolist()) == set(range(1, 17))
        _CASES[key] = t
    return _CASES[key]


# ---------------------------------------------------------------------------------------------------- dequantising transpose
@pytest.mark.parametrize("K,N,g", [(128, 64, 32), (128, 192, 128), (256, 200, 64), (136 * 8, 72, -1), (4096, 12288, 128)])
def test_dequant_kernel_is_exact(hip, K, N, g):
    """one group only, a partial last N tile, an N that is a multiple of 8 but not of the tile, group_size -1, one true-width matrix"""
    t = packed_case(K, N, g)
    W = nan_like((N, K), torch.bfloat16)
    hip.call("vlr_gptq_dequant_bf16", t["qweight"], t["qzeros"], t["scales"], W, K, N, R.group(K, g))
    torch.cuda.synchronize()
    assert torch.equal(W, t["W"])
    assert float(W[1].float().min()) != float(W[2].float().max())          # the all-15 and the all-0 column are both in there


# ---------------------------------------------------------------------------------------------------- packed skinny GEMM
def gemv_w4(hip, mode, X, t, g, Y, M, N, K, bias=None, res=None, ldr=0, pos=None, cos=None, sin=None, rope_cols=0, hd=128, max_pos=0):
    ws = torch.empty(int(hip.lib().vlr_gemv_w4_workspace_bytes(M, N, K)), dtype=torch.uint8, device=DEV)
    hip.call("vlr_gemv_w4", mode, X, X.shape[1], t["qweight"], t["qzeros"], t["scales"], R.group(K, g), Y, Y.shape[1], bias, res, ldr, pos,
             cos, sin, rope_cols, hd, max_pos, M, N, K, ws)


def gemv_bf16(hip, mode, X, W, Y, M, N, K, bias=None, res=None, ldr=0, pos=None, cos=None, sin=None, rope_cols=0, hd=128, max_pos=0):
    ws = torch.empty(int(hip.lib().vlr_gemv_workspace_bytes(M, N, K)), dtype=torch.uint8, device=DEV)
    hip.call("vlr_gemv_bf16", mode, X, X.shape[1], W, Y, Y.shape[1], bias, res, ldr, pos, cos, sin, rope_cols, hd, max_pos, M, N, K, ws)


def rnd(*shape, scale=1.0, seed=0, dtype=torch.bfloat16):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


@pytest.mark.parametrize("g", [32, 128])
@pytest.mark.parametrize("K,N", [(128, 192), (256, 192), (4096, 4096), (11008, 4096)])
@pytest.mark.parametrize("M", [1, 3, 16])
def test_gemv_w4_plain(hip, M, K, N, g):
    """Y = X W^T with W read packed, bf16 and fp32 out, against fp32 torch on the dequantised matrix (the bounds of vlr_gemv_bf16's own
    test); the fp32 result is bit-identical run to run"""
    t = packed_case(K, N, g)
    X = rnd(M, K, seed=1)
    ref = X.float() @ t["W"].float().T
    Y = nan_like((M, N), torch.bfloat16)
    gemv_w4(hip, hip.GEMV_BF16, X, t, g, Y, M, N, K)
    F = nan_like((M, N), torch.float32)
    gemv_w4(hip, hip.GEMV_F32, X, t, g, F, M, N, K)
    F2 = nan_like((M, N), torch.float32)
    gemv_w4(hip, hip.GEMV_F32, X, t, g, F2, M, N, K)
    torch.cuda.synchronize()
    check(Y, ref, 8e-3, "bf16 out")
    check(F, ref, 1e-4, "fp32 out")
    assert torch.equal(F, F2)


def test_gemv_w4_bias_residual_matches_bf16_kernel(hip):
    M, K, N, g = 3, 4096, 4096, 128
    t = packed_case(K, N, g)
    X, bias, res = rnd(M, K, seed=3), rnd(N, seed=5), rnd(M, N, seed=6)
    Y, Yb = nan_like((M, N), torch.bfloat16), nan_like((M, N), torch.bfloat16)
    gemv_w4(hip, hip.GEMV_BF16, X, t, g, Y, M, N, K, bias=bias, res=res, ldr=N)
    gemv_bf16(hip, hip.GEMV_BF16, X, t["W"], Yb, M, N, K, bias=bias, res=res, ldr=N)
    torch.cuda.synchronize()
    check(Y, Yb, 8e-3, "bias + residual vs vlr_gemv_bf16")


def test_gemv_w4_qkv_rope_matches_bf16_kernel(hip):
    M, H, nh, nkv, hd, max_pos, g = 3, 256, 2, 1, 128, 4096, 32
    N, rc = (nh + 2 * nkv) * hd, (nh + nkv) * hd
    t = packed_case(H, N, g)
    cos = torch.empty(max_pos, hd // 2, dtype=torch.float32, device=DEV)
    sin = torch.empty_like(cos)
    hip.call("vlr_rope_table", cos, sin, max_pos, hd, 10000.0)
    X, b = rnd(M, H, seed=8), rnd(N, seed=10)
    pos = torch.tensor([(37 * i + 5) % 3000 for i in range(M)], dtype=torch.int32, device=DEV)
    Y, Yb = nan_like((M, N), torch.bfloat16), nan_like((M, N), torch.bfloat16)
    gemv_w4(hip, hip.GEMV_QKV_ROPE, X, t, g, Y, M, N, H, bias=b, pos=pos, cos=cos, sin=sin, rope_cols=rc, hd=hd, max_pos=max_pos)
    gemv_bf16(hip, hip.GEMV_QKV_ROPE, X, t["W"], Yb, M, N, H, bias=b, pos=pos, cos=cos, sin=sin, rope_cols=rc, hd=hd, max_pos=max_pos)
    torch.cuda.synchronize()
    check(Y, Yb, 8e-3, "q|k|v + bias + RoPE vs vlr_gemv_bf16")


# ---------------------------------------------------------------------------------------------------- the engine over a packed base
def llava_pair(tmp_path, g=32):
    """A = from_pretrained of the written GPTQ checkpoint (packed); B = the bf16 engine on the host-dequantised weights"""
    from vlrlhf.models.Llava import LlavaForRL, _hf_from_cfg
    z, cfg, W, W_ref, batch, rows = load_case("llava_hipsmall")
    deq = R.write_checkpoint(str(tmp_path), _hf_from_cfg(cfg), W, g)
    A = LlavaForRL.from_pretrained(str(tmp_path))
    assert A.is_packed and A.engine.cfg["gptq"]["group_size"] == g
    B = LlavaForRL.from_state_dict({k: v for k, v in A.engine.cfg.items() if k != "gptq"}, deq)
    assert not B.is_packed
    return cfg, batch, A, B


def llava_trainer(model, cfg):
    from vlrlhf.models.Llava import LlavaDPOTrainer
    o = cfg["optim"]
    args = SimpleNamespace(gradient_accumulation_steps=1, per_device_train_batch_size=2, learning_rate=o["lr"], adam_beta1=o["beta1"],
                           adam_beta2=o["beta2"], adam_epsilon=o["eps"], weight_decay=o["weight_decay"], max_grad_norm=o["max_grad_norm"], seed=0)
    return LlavaDPOTrainer(model, None, cfg["beta"], 0, "sigmoid", args, None, -100, 0, "keep_end", None, None, None, peft_config=dict(PEFT))


def wake_adapters(eng):
    for k, t in eng.lv.items():                      # peft init has B = 0: give the adapters something to do
        if ".b_" in k:
            t.copy_(torch.randn(t.shape, generator=torch.Generator().manual_seed(len(k))).mul(0.02))


def three_steps(tr, model, batch, o):
    eng = model.engine
    eng.init_optimizer()
    model.train()
    losses = []
    for _ in range(3):
        losses.append(float(tr.training_step(model, batch)))
        eng.optimizer_step(o["lr"], o["beta1"], o["beta2"], o["eps"], o["weight_decay"], o["max_grad_norm"])
    torch.cuda.synchronize()
    return losses, {k: v.clone() for k, v in model.lora_state_dict().items()}


@pytest.mark.parametrize("ckpt", [False, True])
def test_llava_q_lora_is_bit_identical_to_bf16_on_dequantised_weights(hip, tmp_path, ckpt):
    cfg, batch, A, B = llava_pair(tmp_path)
    # the persistent packed tensors: qweight + qzeros + scales = 4.625 bits per weight at g = 32, against 16
    dense = sum(p.N * p.K * 2 for p in A.engine.packed.values())
    assert dense == sum(B.engine.policy.v[n].numel() * 2 for n in A.engine.packed)
    assert A.engine.packed_nbytes() <= 0.30 * dense, (A.engine.packed_nbytes(), dense)
    assert A.engine.policy.flat.numel() + dense // 2 == B.engine.policy.flat.numel()      # no packed entry takes room in the flat buffer
    ta, tb = llava_trainer(A, cfg), llava_trainer(B, cfg)
    for m in (A, B):
        wake_adapters(m.engine)
        if ckpt:
            m.gradient_checkpointing_enable()
    if not ckpt:
        for m in (A, B):
            m.eval()
        with torch.no_grad():
            pa, pb = ta.concatenated_forward(A, batch), tb.concatenated_forward(B, batch)
            with A.disable_adapter():
                ra = ta.concatenated_forward(A, batch)
            with B.disable_adapter():
                rb = tb.concatenated_forward(B, batch)
        assert torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1]), "policy log-probs"
        assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1]), "reference (adapter-off) log-probs"
        assert not torch.equal(pa[0], ra[0])
    la, sa = three_steps(ta, A, batch, cfg["optim"])
    lb, sb = three_steps(tb, B, batch, cfg["optim"])
    assert la == lb, (la, lb)
    assert len(set(la)) > 1                          # the adapters move
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    with pytest.raises(NotImplementedError, match="GPTQ"):
        A.merge_and_unload()
    with pytest.raises(NotImplementedError, match="save_adapter"):
        A.save_pretrained(str(tmp_path / "whole"))
    if not ckpt:                                      # the adapter round-trips through its file as on a bf16 base
        A.save_adapter(str(tmp_path / "adapter"))
        B.load_adapter(str(tmp_path / "adapter"))
        assert all(torch.equal(v, B.lora_state_dict()[k]) for k, v in sa.items())


def test_auto_load_rlmodel_q_lora_on_the_device(hip, tmp_path):
    from vlrlhf.models.Llava import _hf_from_cfg
    from vlrlhf.utils.auto_load import auto_load_rlmodel
    z, cfg, W, W_ref, batch, rows = load_case("llava_hipsmall")
    R.write_checkpoint(str(tmp_path), _hf_from_cfg(cfg), W, 32)
    model, ref, lora = auto_load_rlmodel(
        SimpleNamespace(model_name_or_path=str(tmp_path), label_pad_token_id=-100, freeze_vision_tower=True), SimpleNamespace(use_lora=True, seed=1),
        SimpleNamespace(q_lora=True, bits=4, lora_r=8, lora_alpha=16, lora_dropout=0.0, lora_target_modules="auto", lora_bias="none", modules_to_save=None))
    assert ref is None and model.is_packed and lora["r"] == 8
    model.apply_lora(lora)
    assert all(".lora_" in n for n, _ in model.named_parameters())


def test_qwenvl_q_lora_is_bit_identical_to_bf16_on_dequantised_weights(hip, tmp_path):
    """the fused biased c_attn and the w1 / w2 order: forward equality and one optimizer step"""
    from vlrlhf.models.QwenVL import QwenVLDPOTrainer, QwenVLForRL, _hf_from_cfg
    z, cfg, W, W_ref, batch, _ = load_case("qwenvl_small")
    deq = R.write_checkpoint(str(tmp_path), _hf_from_cfg(dict(cfg, family="qwen_vl")), W, 32)
    A = QwenVLForRL.from_pretrained(str(tmp_path))
    B = QwenVLForRL.from_state_dict({k: v for k, v in A.engine.cfg.items() if k != "gptq"}, deq)
    assert A.is_packed and not B.is_packed and any(n.endswith(".bqkv") for n in A.engine.policy.v)
    peft = dict(r=8, lora_alpha=16, lora_dropout=0.05, target_modules="auto", bias="none", seed=5)
    trs = [QwenVLDPOTrainer(m, None, cfg["beta"], 0, "sigmoid", SimpleNamespace(gradient_accumulation_steps=1), None, -100, cfg["pad_token_id"],
                            peft_config=dict(peft)) for m in (A, B)]
    outs = []
    for m, tr in zip((A, B), trs):
        wake_adapters(m.engine)
        m.eval()
        with torch.no_grad():
            fwd = tr.concatenated_forward(m, batch)
        m.train()
        m.engine.init_optimizer()
        loss = float(tr.training_step(m, batch))
        m.engine.optimizer_step(lr=1e-3, beta1=0.9, beta2=0.98, eps=1e-6, weight_decay=0.05, max_grad_norm=1.0)
        torch.cuda.synchronize()
        outs.append((fwd, loss, {k: v.clone() for k, v in m.lora_state_dict().items()}))
    assert torch.equal(outs[0][0][0], outs[1][0][0]) and torch.equal(outs[0][0][1], outs[1][0][1])
    assert outs[0][1] == outs[1][1]
    for k, v in outs[0][2].items():
        assert torch.equal(v, outs[1][2][k]), k


def test_decode_from_packed_weights(hip, tmp_path):
    """prefill logits bit-identical (the prefill dequantises); then 8 teacher-forced decode steps on B's greedy tokens: A's logits within
    1e-4 relative of B's (same bf16 products, fp32 sums in another order); generate(use_cache=True) runs on the packed model"""
    cfg, batch, A, B = llava_pair(tmp_path)
    ids, mask = batch["prompt_input_ids"].to(DEV), batch["prompt_attention_mask"].to(DEV)
    pv = batch["img_input_dict"]["pixel_values"].to(DEV)
    Bn, T = ids.shape
    Tp = (T + 31) // 32 * 32
    fill = torch.zeros(Bn, Tp - T, dtype=ids.dtype, device=DEV)
    run_ids, run_mask = torch.cat([fill, ids], 1), torch.cat([torch.zeros_like(fill), mask], 1)
    steps = 8
    logits, caches = [], []
    for m in (A, B):
        m.eval()
        eng = m.engine
        cache = eng.new_kv_cache(Bn, steps + 1)
        with torch.no_grad():
            c = eng.forward_hidden(m.weights, run_ids, run_mask, None, pv, save=False, tag="policy_ng", kv_cache=cache)
            logits.append(m._last_logits(c, Bn, m.weights.v["lm_head"]).clone())
        caches.append(cache)
    assert torch.equal(logits[0], logits[1]), "prefill logits"
    calls = []
    call = hip.call
    la = logits[1]
    try:
        hip.call = lambda name, *a: (calls.append(name), call(name, *a))[1]
        for k in range(steps):
            tok = la.argmax(-1)                       # B's greedy token feeds both models
            with torch.no_grad():
                xa = A.engine.decode_step(A.weights, tok, caches[0])
                la = B.engine.decode_step(B.weights, tok, caches[1])
            torch.cuda.synchronize()
            check(xa, la, 1e-4, f"decode step {k}")
    finally:
        hip.call = call
    assert calls.count("vlr_decoder_layer_decode_w4") == calls.count("vlr_decoder_layer_decode") == steps * A.engine.L
    assert "vlr_gptq_dequant_bf16" not in calls       # decoding streams the packed weights
    new = 5
    out = A.generate(input_ids=ids, attention_mask=mask, pixel_values=pv, max_new_tokens=new, do_sample=False, pad_token_id=0,
                     eos_token_id=10 ** 6, use_cache=True)
    assert out.shape == (Bn, T + new) and torch.equal(out[:, :T], ids)
