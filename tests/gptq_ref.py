"""Reference side of the GPTQ int4 tests: plain torch and numpy, nothing imported from the package under test.

Format (AutoGPTQ "v1"), for a linear y = x W^T, W [N][K], group size g:
    qweight int32 [K/8][N]    nibble j (bits 4j .. 4j+3) of qweight[k8][n] = q[8 k8 + j][n]
    qzeros  int32 [K/g][N/8]  nibble j of qzeros[G][n8] = stored zero of column 8 n8 + j; zero used = stored + 1 (15 -> 16)
    scales  fp16  [K/g][N]
    g_idx   int32 [K]         k // g
    W[n][k] = bf16_rne(float(scales[k//g][n]) * float(q[k][n] - zero[k//g][n]))"""
import json
import os
import re

import numpy as np
import torch

# decoder projections of the supported checkpoints (LLaVA / LLaVA-Next: language_model.model.layers.N.*; Qwen-VL: transformer.h.N.*)
DECODER_LINEAR = re.compile(r"^(language_model\.model\.layers|transformer\.h)\.\d+\.(self_attn\.[qkvo]_proj|mlp\.(gate|up|down)_proj|"
                            r"attn\.c_attn|attn\.c_proj|mlp\.w1|mlp\.w2|mlp\.c_proj)\.weight$")


def group(K, g):
    return K if g == -1 else g


def quantize_rtn(W, g):
    """per-group asymmetric round-to-nearest of W [N][K] -> q [K][N] in 0..15, zero [K/g][N] in 1..16, scales fp16 [K/g][N]"""
    W = W.float()
    N, K = W.shape
    g = group(K, g)
    w = W.t().reshape(K // g, g, N)
    lo, hi = w.min(1).values.clamp(max=0), w.max(1).values.clamp(min=0)
    scales = ((hi - lo) / 15).clamp(min=1e-6).half()
    s = scales.float()
    zero = torch.round(-lo / s).clamp(1, 16).to(torch.int32)
    q = (torch.round(w / s[:, None]) + zero[:, None]).clamp(0, 15).to(torch.int32).reshape(K, N)
    return q, zero, scales


def pack(q, zero, scales, g):
    """-> dict(qweight, qzeros, scales, g_idx) in the checkpoint format"""
    K, N = q.shape
    g = group(K, g)
    assert K % 8 == 0 and N % 8 == 0 and int(q.min()) >= 0 and int(q.max()) <= 15 and int(zero.min()) >= 1 and int(zero.max()) <= 16
    sh = (np.arange(8, dtype=np.uint32) * 4)
    qn = q.numpy().astype(np.uint32).reshape(K // 8, 8, N)
    qweight = np.bitwise_or.reduce(qn << sh[None, :, None], axis=1)
    zn = (zero.numpy().astype(np.uint32) - 1).reshape(K // g, N // 8, 8)
    qzeros = np.bitwise_or.reduce(zn << sh[None, None, :], axis=2)
    return dict(qweight=torch.from_numpy(qweight.view(np.int32).copy()), qzeros=torch.from_numpy(qzeros.view(np.int32).copy()),
                scales=scales.half().contiguous(), g_idx=(torch.arange(K) // g).to(torch.int32))


def dequant(qweight, qzeros, scales, g):
    """the four tensors -> W bf16 [N][K] by the one definition of the format (on the tensors' own device)"""
    dev = qweight.device
    K, N = qweight.shape[0] * 8, qweight.shape[1]
    g = group(K, g)
    sh = torch.arange(8, dtype=torch.int32, device=dev) * 4
    q = ((qweight[:, None, :] >> sh[None, :, None]) & 15).reshape(K, N)            # nibble j of row k8 = k 8 k8 + j
    z = ((qzeros[:, :, None] >> sh[None, None, :]) & 15).reshape(K // g, N) + 1    # nibble j of word n8 = column 8 n8 + j; + 1, no wrap
    grp = torch.arange(K, device=dev) // g
    w = scales.float()[grp] * (q - z[grp]).float()                                 # exact in fp32
    return w.to(torch.bfloat16).t().contiguous()


def quantize_state_dict(state_dict, g):
    """-> (packed checkpoint state dict, the same model with every decoder projection replaced by its dequantised bf16 weight).
    Everything that is not a decoder projection is rounded to bf16 in both."""
    packed, deq = {}, {}
    for k, v in state_dict.items():
        if DECODER_LINEAR.match(k):
            t = pack(*quantize_rtn(v, g), g)
            for n, x in t.items():
                packed[k[:-len("weight")] + n] = x
            deq[k] = dequant(t["qweight"], t["qzeros"], t["scales"], g)
        else:
            packed[k] = deq[k] = v.to(torch.bfloat16)
    return packed, deq


def write_checkpoint(path, cfg, state_dict, g, **quant):
    """a GPTQ checkpoint directory: config.json = `cfg` (the model's HF config) + quantization_config, model.safetensors = the packed
    decoder projections and everything else in bf16.  -> the dequantised bf16 state dict of the same model"""
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    packed, deq = quantize_state_dict(state_dict, g)
    hf = dict(cfg)
    hf["quantization_config"] = dict(dict(quant_method="gptq", bits=4, group_size=g, desc_act=False, sym=False, damp_percent=0.01,
                                          true_sequential=True), **quant)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(hf, f)
    save_file({k: v.contiguous() for k, v in packed.items()}, os.path.join(path, "model.safetensors"))
    return deq
