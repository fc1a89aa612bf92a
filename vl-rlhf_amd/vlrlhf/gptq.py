"""GPTQ int4 base weights for q_lora (reference utils/auto_load.py:520-548: GPTQConfig(bits, disable_exllama=True) under a LoRA
adapter).  Host side only: reading the checkpoint's `quantization_config`, validating what the HIP kernels take, and re-laying the
packed tensors of the decoder projections into the engine's fused row order.  No GPTQ package is needed: the checkpoint format
(AutoGPTQ "v1") is, for a linear y = x W^T with W [N][K] and group size g,

    qweight int32 [K/8][N]    nibble j (bits 4j .. 4j+3) of qweight[k8][n] = q[8 k8 + j][n], 0 .. 15
    qzeros  int32 [K/g][N/8]  nibble j of qzeros[G][n8] = STORED zero of column 8 n8 + j; the zero used is stored + 1 (15 -> 16)
    scales  fp16  [K/g][N]
    g_idx   int32 [K]         k // g (anything else is act-order, refused)
    W[n][k] = bf16_rne(float(scales[k//g][n]) * float(q[k][n] - zero[k//g][n]))

The fp32 product is exact, so there is exactly one rounding: `dequant` below, vlr_gptq_dequant_bf16 and vlr_gemv_w4 (include/vlr.h)
agree bit for bit."""
import re

import torch

PACKED_KEYS = ("qweight", "qzeros", "scales", "g_idx")
DECODER_LINEARS = ("wqkv", "wo", "wgu", "wdown")      # ParamLayout entry suffixes that are packed under GPTQ


def parse_quantization_config(hf_config):
    """config.json -> dict(bits=4, group_size) for a GPTQ checkpoint, None for an unquantised one; everything the kernels do not take
    is refused with its own message"""
    qc = (hf_config or {}).get("quantization_config")
    if not qc:
        return None
    method = str(qc.get("quant_method", "gptq")).lower()
    if method != "gptq":
        raise NotImplementedError(f"quantization_config.quant_method {method!r}: only GPTQ checkpoints load packed on the MI355X path")
    bits = int(qc.get("bits", 4))
    if bits != 4:
        raise NotImplementedError(f"GPTQ bits={bits}: the MI355X kernels unpack 4-bit weights only")
    if str(qc.get("checkpoint_format", "gptq")).lower() == "gptq_v2":
        raise NotImplementedError("GPTQ checkpoint_format 'gptq_v2' (zeros stored without the +1 offset) is not supported; "
                                  "export the checkpoint in the v1 format")
    return dict(bits=4, group_size=int(qc.get("group_size", 128)), desc_act=bool(qc.get("desc_act", False)), sym=bool(qc.get("sym", True)))


def group_size_for(K, group_size):
    """the group size in elements (-1 = one group over all of K), validated against what the kernels take"""
    g = K if group_size == -1 else int(group_size)
    if g != K and (g < 32 or g % 32 or K % g):
        raise ValueError(f"GPTQ group_size {group_size}: must be -1 or a multiple of 32 that divides K = {K}")
    return g


def unpack_nibbles(words, dim):
    """int32 tensor -> the 8 nibbles of every word expanded along `dim` (nibble j = bits 4j .. 4j+3), int32 in 0 .. 15"""
    sh = torch.arange(8, dtype=torch.int32, device=words.device) * 4
    w = words.to(torch.int32)
    if dim == 0:
        return ((w.unsqueeze(1) >> sh.view(1, 8, 1)) & 15).reshape(-1, w.shape[1])
    return ((w.unsqueeze(2) >> sh.view(1, 1, 8)) & 15).reshape(w.shape[0], -1)


def dequant(qweight, qzeros, scales, group_size):
    """packed -> W bf16 [N][K] by the one rule of the format"""
    q = unpack_nibbles(qweight, 0)                     # [K][N]
    K = q.shape[0]
    g = group_size_for(K, group_size)
    zero = unpack_nibbles(qzeros, 1) + 1               # [K/g][N], 1 .. 16
    grp = torch.arange(K, device=q.device) // g
    w = scales.float()[grp] * (q - zero[grp]).float()
    return w.to(torch.bfloat16).t().contiguous()


class PackedLinear:
    """one fused decoder projection, packed: qweight [K/8][N] int32, qzeros [K/g][N/8] int32, scales [K/g][N] fp16"""

    def __init__(self, qweight, qzeros, scales, group_size):
        self.qweight, self.qzeros, self.scales = qweight.contiguous(), qzeros.contiguous(), scales.contiguous()
        self.K, self.N = self.qweight.shape[0] * 8, self.qweight.shape[1]
        self.g = group_size_for(self.K, group_size)
        if self.N % 8:
            raise ValueError(f"GPTQ linear with N = {self.N} output features: N must be a multiple of 8")
        if tuple(self.qzeros.shape) != (self.K // self.g, self.N // 8) or tuple(self.scales.shape) != (self.K // self.g, self.N):
            raise ValueError(f"GPTQ linear [{self.N}][{self.K}], group {self.g}: qzeros {tuple(self.qzeros.shape)} / scales "
                             f"{tuple(self.scales.shape)} do not match the format")

    def to(self, device):
        return PackedLinear(self.qweight.to(device), self.qzeros.to(device), self.scales.to(device), self.g)

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.qweight, self.qzeros, self.scales))

    def dequant(self):
        return dequant(self.qweight, self.qzeros, self.scales, self.g)


def _read_linear(sd, prefix, group_size):
    """the packed tensors of checkpoint module `prefix` (validated) -> PackedLinear"""
    try:
        qw, qz, sc = (sd[f"{prefix}.{k}"] for k in PACKED_KEYS[:3])
    except KeyError as e:
        raise KeyError(f"GPTQ checkpoint: missing {e.args[0]}") from None
    if qw.dtype != torch.int32 or qz.dtype != torch.int32:
        raise ValueError(f"{prefix}: qweight / qzeros must be int32")
    lin = PackedLinear(qw, qz, sc.to(torch.float16), group_size)
    g_idx = sd.get(f"{prefix}.g_idx")
    if g_idx is not None and not torch.equal(g_idx.to(torch.int64).cpu(), torch.arange(lin.K) // lin.g):
        raise NotImplementedError(f"{prefix}: g_idx is not k // group_size (desc_act with a permuted g_idx is not supported: "
                                  "the packed kernels read the groups in order)")
    return lin


def fuse(parts):
    """PackedLinears of the same K and group size stacked along N in the given order (q|k|v, gate|up): the bf16 loader's row order.
    Every part has N % 8 == 0, so the qzeros words stack whole."""
    if len(parts) == 1:
        return parts[0]
    return PackedLinear(torch.cat([p.qweight for p in parts], 1), torch.cat([p.qzeros for p in parts], 1),
                        torch.cat([p.scales for p in parts], 1), parts[0].g)


_ENTRY = re.compile(r"^l\d+\.(%s)$" % "|".join(DECODER_LINEARS))


def is_packed_entry(name):
    return _ENTRY.match(name) is not None


def load_packed_decoder(sd, layout, group_size):
    """checkpoint state dict -> {ParamLayout entry ("l3.wqkv", ...): PackedLinear} for every decoder projection, in the engine's fused
    row order: the parts of an entry are stacked in the order (and at the row offsets) the bf16 loader copies them."""
    out = {}
    for name, shape, parts in layout.entries:
        if not is_packed_entry(name):
            continue
        if layout.row_perm.get(name) is not None:
            raise NotImplementedError(f"{name}: packed weights with a row re-ordering are not supported")
        lins, row = [], 0
        for hf, r0, rows in parts:
            assert r0 == row, (name, hf, r0, row)
            lin = _read_linear(sd, hf[:-len(".weight")], group_size)
            if lin.N != rows or lin.K != shape[1]:
                raise ValueError(f"{hf}: packed shape [{lin.N}][{lin.K}] does not match the model's [{rows}][{shape[1]}]")
            lins.append(lin)
            row += rows
        out[name] = fuse(lins)
    return out
