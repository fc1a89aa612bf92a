"""Host replay (numpy) of the NEFTune noise of include/vlr.h vlr_neftune_add: Philox4x32-10 as published (Salmon, Moraes, Dror, Shaw:
"Parallel random numbers: as easy as 1, 2, 3", SC'11) and the word -> value construction, bit for bit."""
import numpy as np
import torch

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85          # Weyl key increments
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """ten rounds on the counter (c0, c1, c2, c3) with the key (k0, k1); the arguments broadcast -> four uint32 arrays"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _MASK for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & _MASK, (k1 + np.uint64(PHILOX_W1)) & _MASK
    return tuple(np.broadcast_arrays(*(c.astype(np.uint32) for c in (c0, c1, c2, c3))))


def noise_words(tok, H, key, call, npass):
    """uint32 [len(tok)][H]: column c of token `tok` is word c % 4 of the block with counter (c / 4, tok, call, pass)"""
    tok = np.asarray(tok, dtype=np.uint64).reshape(-1, 1)
    blk = np.arange(H // 4, dtype=np.uint64).reshape(1, -1)
    w = philox4x32_10(blk, tok, call, npass, int(key) & 0xFFFFFFFF, int(key) >> 32)
    return np.stack(w, axis=-1).reshape(tok.shape[0], H)


def noise(tok, H, scale, key, call, npass):
    """fp32 [len(tok)][H]: the top 24 bits r of each word -> h = r - 8388607.5 (exact), n = h * scale rounded to fp32 once"""
    r = (noise_words(tok, H, key, call, npass) >> np.uint32(8)).astype(np.float32)
    return (r - np.float32(8388607.5)) * np.float32(scale)


def bf16_bits(f):
    """fp32 array -> bf16 bit patterns, round to nearest even (finite values)"""
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def add_noise(x, src, T, nf):
    """the expected output of vlr_neftune_add: x [Bn*S][H] torch tensor (fp32 or bf16, any device) with the noise of
    nf = (key, call, pass, T, scale) on the rows whose src [Bn][S] entry is >= 0; every other row untouched -> CPU tensor of x's dtype"""
    key, call, npass, _, scale = nf
    x = x.detach().cpu()
    src = np.asarray(src.detach().cpu().numpy() if isinstance(src, torch.Tensor) else src)
    Bn, S = src.shape
    H = x.shape[-1]
    flat = src.reshape(-1)
    rows = np.nonzero(flat >= 0)[0]
    tok = (rows // S) * T + flat[rows]
    rows = torch.from_numpy(rows)
    n = noise(tok, H, scale, key, call, npass)
    out = x.clone().reshape(Bn * S, H)
    if x.dtype == torch.float32:
        out[rows] = torch.from_numpy(out[rows].numpy() + n)
    else:
        s = out[rows].float().numpy() + n                     # the fp32 sum, then one rounding to bf16
        out[rows] = torch.from_numpy(bf16_bits(s).view(np.int16).copy()).view(torch.bfloat16)
    return out.reshape(x.shape)
