"""The fused-epilogue GEMMs of csrc/gemm256p.hip element by element at their tile edges: every case of tests/fused_gemm_ref.py through
the C ABI (vlr_gemm_swiglu[_lora], vlr_gemm_qkv_rope[_bias | _lora], vlr_gemm_swiglu_bwd[_add]) against the float64 reference of the
route the case takes - bitwise where the exact regimes promise bits, an elementwise bound elsewhere - with NaN in the operands' padding,
NaN guards and guard rows around every buffer, every cell outside the logical results compared after the run, the route asserted from the
gemm256p launches the in-library profiler counts (1 = fused, 0 = the fallback of include/vlr.h), the operands checked to be read only, and
every case run twice for bit-identical results.  The multi-tile cases run a third time under vlr_gemm_set_sched(16): the same bits.
tests/test_fused_gemm_checker_host.py runs the same checker on the CPU.  Needs a real MI355X: pytest -m gpu"""
import pytest
import torch

from tests import fused_gemm_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return _hip


class Run:
    """one case on the GPU: the operands with their NaN padding, guards and guard rows (g), the entry point's arguments"""

    def __init__(self, hip, c):
        self.c = c
        self.inp = R.make(c)
        if c.op == "rope" and c.tables == "device":          # the tables vlr_rope_table writes, read back: float inputs of the case
            half = c.hd // 2
            cos = torch.empty(R.MAX_POS, half, dtype=torch.float32, device=DEV)
            sin = torch.empty_like(cos)
            hip.call("vlr_rope_table", cos, sin, R.MAX_POS, c.hd, 10000.0)
            torch.cuda.synchronize()
            R.logical(self.inp["cos"])[:] = cos.cpu()
            R.logical(self.inp["sin"])[:] = sin.cpu()
        self.g = {k: (b if k == "pos" else b.flat).to(DEV) for k, b in self.inp.items()}
        self.first = {k: self.g[k].clone() for k in R.outputs(c)}

    def at(self, k):
        if k not in self.g:
            return None
        return self.g[k] if k == "pos" else self.g[k][self.inp[k].off:]

    def reset(self):
        for k, t in self.first.items():
            self.g[k].copy_(t)

    def launch(self, hip):
        c, at = self.c, self.at
        if c.op == "swiglu":
            if c.r:
                hip.call("vlr_gemm_swiglu_lora", at("x"), at("W"), at("gu"), at("act"), c.M, c.I, c.K, c.ldx, at("u"), c.ldu, at("Bl"), c.r)
            else:
                hip.call("vlr_gemm_swiglu", at("x"), at("W"), at("gu"), at("act"), c.M, c.I, c.K, c.ldx, c.store_gu)
        elif c.op == "rope":
            tail = (at("qkv"), at("pos"), at("cos"), at("sin"), c.M, c.N, c.rope_cols, c.K, c.ldx, c.hd, R.MAX_POS)
            if c.r:
                hip.call("vlr_gemm_qkv_rope_lora", at("x"), at("W"), at("bias"), *tail, at("u"), c.ldu, at("Bl"), c.r, *c.qkv_cols)
            elif c.bias is None:
                hip.call("vlr_gemm_qkv_rope", at("x"), at("W"), *tail)
            else:
                hip.call("vlr_gemm_qkv_rope_bias", at("x"), at("W"), at("bias"), *tail)
        elif c.add:
            hip.call("vlr_gemm_swiglu_bwd_add", at("dy"), at("W"), at("gu"), at("ws"), at("add" if c.add == "sep" else "ws"), c.M, c.I, c.K)
        else:
            hip.call("vlr_gemm_swiglu_bwd", at("dy"), at("W"), at("gu"), at("ws"), c.M, c.I, c.K)

    def outs(self):
        torch.cuda.synchronize()
        return {k: self.g[k].clone() for k in R.outputs(self.c)}


def same(a, b):
    return all(torch.equal(R.row_bits(a[k]), R.row_bits(b[k])) for k in a)


def run_case(hip, c, say=print):
    r = Run(hip, c)
    assert R.entry(c) in hip.exported_symbols()
    torch.cuda.synchronize()
    try:
        hip.lib_profile_start(1)
        r.launch(hip)
        n256 = hip.lib_profile_stop()["gemm256p"][0]
        first = r.outs()
        r.reset()
        r.launch(hip)
        second = r.outs()
        third = None
        if R.is_multi(c):                                     # "bit-identical results" under the serial epilogue order
            assert hip.helper("vlr_gemm_set_sched", 16) == 0
            r.reset()
            r.launch(hip)
            third = r.outs()
    finally:
        torch.cuda.synchronize()
        hip.helper("vlr_gemm_set_sched", -1)
    assert n256 == c.n256, f"{c.name}: {n256} launches of gemm256p_kernel, expected {c.n256} ({'fused' if c.n256 else 'fallback'})"
    assert same(first, second), f"{c.name}: two runs differ"
    assert third is None or same(first, third), f"{c.name}: vlr_gemm_set_sched(16) changes bits"
    for k in r.g:                                             # the operands are read only
        if k not in first:
            host = r.inp[k] if k == "pos" else r.inp[k].flat
            assert torch.equal(R.row_bits(r.g[k].cpu()), R.row_bits(host)), f"{c.name}: operand {k} was written"
    exp = R.expect(c, r.inp, DEV if R.macs(c) > R.DEVICE_REF_MACS else "cpu")
    exp = {k: R.Exp(e.ref.cpu(), None if e.mag is None else e.mag.cpu(), e.rel, e.coef) for k, e in exp.items()}
    after = {k: v.cpu() for k, v in first.items()}
    for k, ratio in R.worst(c, r.inp, after, exp).items():
        say(f"{c.name} {k}: worst |error| / bound = {ratio:.3f}")
    R.check_case(c, r.inp, after, exp)


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_fused_gemm_case(hip, name):
    run_case(hip, R.BY_NAME[name])
