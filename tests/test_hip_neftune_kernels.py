"""vlr_neftune_add (csrc/dpo_ops.hip) through the C ABI on the MI355X against the numpy replay of tests/neftune_ref.py, bit for bit, on
both residual-stream types.  Rows the kernel must skip are NaN-poisoned with a marked payload.  Needs a real MI355X:  pytest -m gpu"""
import numpy as np
import pytest
import torch

from tests import neftune_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
Z = -(2 ** 31)              # SRC_ZERO: a merged row that stays zero (left padding, the model's pad token)
BN, T, P = 3, 7, 3          # three rows of seven tokens; an image expands to P = 3 merged rows -> S = T - 1 + P = 9
# src[b][s] >= 0: text token t;  -(f + 1): image-feature row f;  Z: zeros
SRC = {
    # an image at the first, a middle and the last token position
    "first_middle_last": [[-1, -2, -3, 1, 2, 3, 4, 5, 6], [0, 1, 2, -4, -5, -6, 4, 5, 6], [0, 1, 2, 3, 4, 5, -7, -8, -9]],
    # a row without an image (left-padded to S), an image in the middle, an image first with a zeroed pad token inside the text
    "no_image_row": [[Z, Z, 0, 1, 2, 3, 4, 5, 6], [0, 1, -1, -2, -3, 3, 4, 5, 6], [-4, -5, -6, 1, 2, Z, 4, 5, 6]],
}
S = 9
KEY, CALL, PASS = (3 << 32) | 42, 5, 0


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return _hip


def bits(x):
    return x.detach().cpu().contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int16)


def make_x(H, dtype, src, seed=0):
    """text rows: random values; every other row: NaN with the row number in its payload (a kernel that read, rewrote or zeroed it shows)"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(BN * S, H, generator=g) * 0.05).to(dtype)
    skip = torch.tensor(src).reshape(-1) < 0
    if dtype == torch.float32:
        pay = (0x7FC00000 + torch.arange(BN * S, dtype=torch.int32))[:, None].expand(-1, H)
        x.view(torch.int32)[skip] = pay[skip]
    else:
        pay = (0x7FC0 + torch.arange(BN * S, dtype=torch.int16))[:, None].expand(-1, H)
        x.view(torch.int16)[skip] = pay[skip]
    return x, skip


def run(hip, x, src, H, scale, key=KEY, call=CALL, npass=PASS):
    y = x.clone().to(DEV)
    s = torch.tensor(src, dtype=torch.int32, device=DEV)
    hip.call("vlr_neftune_add", y, int(x.dtype == torch.float32), s, BN, T, S, H, scale, key, call, npass)
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("layout", list(SRC))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("H", [64, 2112])          # under one sweep of 256 lanes x 8 columns; one sweep and a partial second
def test_matches_the_replay_bit_for_bit(hip, H, dtype, layout):
    from vlrlhf.engine import neftune_scale
    src = SRC[layout]
    m, scale = neftune_scale(5.0, T, H)
    x, skip = make_x(H, dtype, src)
    y = run(hip, x, src, H, scale)
    exp = R.add_noise(x, np.array(src), T, (KEY, CALL, PASS, T, scale))
    assert torch.equal(bits(y), bits(exp)), f"{int((bits(y) != bits(exp)).sum())} of {y.numel()} values differ from the replay"
    assert torch.equal(bits(y)[skip], bits(x)[skip]), "image-feature / zero rows must stay bit-identical"
    d = (y[~skip].double() - x[~skip].double()).abs()
    ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -24      # half an ulp of the largest |x + n| here (< 1), relative to 1
    assert float(d.max()) < m + ulp and float(d.max()) > 0.9 * m and bool((y[~skip] != x[~skip]).float().mean() > 0.9)
    # the same (key, call, pass) again: the same bits
    assert torch.equal(bits(run(hip, x, src, H, scale)), bits(y))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_stream_depends_on_key_call_and_pass_and_scale_zero_is_the_identity(hip, dtype):
    from vlrlhf.engine import neftune_scale
    H, src = 64, SRC["first_middle_last"]
    scale = neftune_scale(5.0, T, H)[1]
    x, skip = make_x(H, dtype, src, seed=1)
    base = run(hip, x, src, H, scale)
    variants = dict(key_low=dict(key=KEY ^ 1), key_high=dict(key=KEY ^ (1 << 32)), call=dict(call=CALL + 1), npass=dict(npass=PASS + 1))
    outs = {k: run(hip, x, src, H, scale, **kw) for k, kw in variants.items()}
    for k, y in outs.items():
        assert not torch.equal(bits(y)[~skip], bits(base)[~skip]), f"changing {k} must change the noise"
        kw = dict(key=KEY, call=CALL, npass=PASS)
        kw.update(variants[k])
        assert torch.equal(bits(y), bits(R.add_noise(x, np.array(src), T, (kw["key"], kw["call"], kw["npass"], T, scale)))), k
    assert len({bits(y).numpy().tobytes() for y in outs.values()}) == len(outs)
    zero = run(hip, x, src, H, 0.0)
    assert torch.equal(zero[~skip], x[~skip]) and torch.equal(bits(zero)[skip], bits(x)[skip])


def test_value_follows_the_token_not_the_merged_layout(hip):
    """token (b, t) draws the same noise wherever the merge puts it: with x = 0 the output IS the noise; the tokens the two layouts share
    sit at different merged positions and must carry the same values"""
    H = 64
    outs = {}
    for name, src in SRC.items():
        x = torch.zeros(BN * S, H)
        y = run(hip, x, src, H, 2.0 ** -23).reshape(BN, S, H)
        outs[name] = {(b, t): y[b, s] for b in range(BN) for s, t in enumerate(src[b]) if t >= 0}
    a, b = outs.values()
    common = set(a) & set(b)
    assert len(common) >= 14 and all(torch.equal(a[k], b[k]) for k in common)
    assert len({a[k].numpy().tobytes() for k in a}) == len(a), "every token has its own stream"


def test_argument_errors(hip):
    x = torch.zeros(BN * S, 64, device=DEV)
    s = torch.tensor(SRC["first_middle_last"], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="null argument"):
        hip.call("vlr_neftune_add", None, 1, s, BN, T, S, 64, 0.0, KEY, CALL, PASS)
    with pytest.raises(ValueError, match="null argument"):
        hip.call("vlr_neftune_add", x, 1, None, BN, T, S, 64, 0.0, KEY, CALL, PASS)
    with pytest.raises(ValueError, match="H % 8"):
        hip.call("vlr_neftune_add", x, 1, s, BN, T, S, 60, 0.0, KEY, CALL, PASS)
    with pytest.raises(ValueError, match="scale"):
        hip.call("vlr_neftune_add", x, 1, s, BN, T, S, 64, 1.5, KEY, CALL, PASS)
    torch.cuda.synchronize()
    assert not x.any()
