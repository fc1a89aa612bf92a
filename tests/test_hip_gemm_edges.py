"""The GEMM family (csrc/gemm.hip, gemm128p.hip, gemm256p.hip) element by element at its tile, K and route edges: every case of
tests/gemm_ref.py through the C ABI against the float64 reference - bitwise in the exact regime, an elementwise bound in the gauss
regime - with NaN in every operand's padding, NaN guards around every buffer, the result compared cell by cell outside the logical
output, the route each case is meant to take asserted from three observables (gemm256p launches of the in-library profiler, writes to a
NaN-filled split-K workspace, vlr_gemm_peel_rows), and every case run twice for bit-identical results.
tests/test_gemm_checker_host.py runs the same checker on the CPU.  Needs a real MI355X: pytest -m gpu"""
import os
import subprocess
import sys

import pytest
import torch

from tests import gemm_ref as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return _hip


class Run:
    """one case on the GPU: the operands with their NaN padding and guards (g), the entry point's arguments"""

    def __init__(self, c):
        self.c = c
        self.inp = G.make(c)
        self.g = {k: b.flat.to(DEV) for k, b in self.inp.items() if b is not None}
        self.c0 = self.g["C"].clone()

    def at(self, k):
        return self.g[k][self.inp[k].off:] if k in self.g else None

    def launch(self, hip):
        c = self.c
        res, ldr = (self.at("C"), c.ldc) if c.inplace else (self.at("R"), c.ldr)
        shape = (c.M, c.N, c.K, c.lda, c.ldb, c.ldc, ldr)
        if c.entry == "grouped":
            a_rows, b_rows = self.inp["A"].rows // c.groups, self.inp["B"].rows // c.groups
            hip.call("vlr_gemm_grouped", c.layout, self.at("A"), self.at("B"), self.at("C"), c.M, c.N, c.K, c.lda, c.ldb, c.ldc, c.groups,
                     a_rows * c.lda, b_rows * c.ldb, c.N, c.alpha, c.acc, 0, 0, 0.0, 0)
        elif c.entry in ("lora", "lora_f32res"):
            hip.call("vlr_gemm_" + c.entry, self.at("A"), c.lda, self.at("B"), self.at("C"), c.ldc, res, ldr, c.M, c.N, c.K, self.at("U"), c.ldu,
                     self.at("Bl"), c.K2)
        elif c.entry == "f32res":
            hip.call("vlr_gemm_bf16_f32res", c.layout, self.at("A"), self.at("B"), self.at("C"), res, *shape)
        elif c.entry == "scaled":
            hip.call("vlr_gemm_bf16_scaled", c.layout, self.at("A"), self.at("B"), self.at("C"), self.at("bias"), res, *shape, c.act, c.acc, c.f32,
                     c.alpha)
        else:
            assert c.alpha == 1.0
            hip.call("vlr_gemm_bf16", c.layout, self.at("A"), self.at("B"), self.at("C"), self.at("bias"), res, *shape, c.act, c.acc, c.f32)


def restore(hip):
    hip.ensure_splitk_workspace(force=True)
    hip.helper("vlr_gemm_set_sched", -1)
    hip.helper("vlr_set_comm_cus", -1)


def run_case(hip, c, say=print):
    """runs the case twice; asserts the route observables, determinism, the result and the guards"""
    r = Run(c)
    ws = torch.full((c.ws_bytes // 4,), NAN, dtype=torch.float32, device=DEV)      # the reducer may read only what the slices wrote
    torch.cuda.synchronize()
    try:
        assert hip.helper("vlr_gemm_set_splitk_workspace", ws.data_ptr(), ws.numel() * 4) == 0
        if c.comm_cus >= 0:
            assert hip.helper("vlr_set_comm_cus", c.comm_cus) == 0
        if c.sched >= 0:
            assert hip.helper("vlr_gemm_set_sched", c.sched) == 0
        peel = hip.helper("vlr_gemm_peel_rows", c.M, c.N)
        hip.lib_profile_start(1)
        r.launch(hip)
        n256 = hip.lib_profile_stop()["gemm256p"][0]
        torch.cuda.synchronize()
        first = r.g["C"].clone()
        wrote_ws = bool((~torch.isnan(ws)).any())
        r.g["C"].copy_(r.c0)
        ws.fill_(NAN)
        r.launch(hip)
        torch.cuda.synchronize()
        second = r.g["C"].clone()
    finally:
        torch.cuda.synchronize()
        restore(hip)
    assert (n256 > 0) == c.uses_256p, f"{c.name}: {n256} launches of gemm256p_kernel, expected the case {'on' if c.uses_256p else 'off'} it"
    assert wrote_ws == c.split_k, f"{c.name}: split-K workspace {'written' if wrote_ws else 'untouched'}, expected split_k = {c.split_k}"
    assert peel == c.peel_rows, f"{c.name}: vlr_gemm_peel_rows = {peel}, expected {c.peel_rows}"
    assert torch.equal(G.row_bits(first), G.row_bits(second)), f"{c.name}: two runs differ"
    for k in ("A", "B", "R", "bias", "U", "Bl"):       # the operands are read-only
        if k in r.g:
            assert torch.equal(G.row_bits(r.g[k].cpu()), G.row_bits(r.inp[k].flat)), f"{c.name}: operand {k} was written"
    e = G.expect(c, r.inp, DEV if G.macs(c) > G.DEVICE_REF_MACS else "cpu")
    e = G.Exp(e.ref.cpu(), None if e.mag is None else e.mag.cpu(), e.rel, e.coef)
    after = first.cpu()
    if e.rel is not None:
        say(f"{c.name}: worst |error| / bound = {G.worst_ratio(after, r.inp['C'], e):.3f}")
    G.check(c.name, after, r.inp["C"], e)


@pytest.mark.parametrize("name", [c.name for c in G.CASES if c.group != "pair"])
def test_gemm_case(hip, name):
    run_case(hip, G.BY_NAME[name])


def test_schedules_are_bit_identical_on_gauss_data(hip):
    """the exact-regime sched0 / sched16 / sched32 cases agree through their common reference; here the same on rounded sums, where
    only an unchanged K order keeps the bits: vlr_gemm_set_sched 0, 16 and 32 on one continuous-pipeline launch"""
    c = G.Case(G.BY_NAME["cont-nt-4104x4104x320-exact-sched0"], regime="gauss", name="cont-nt-4104x4104x320-gauss-sched")
    r = Run(c)
    outs = []
    try:
        for mode in (0, 16, 32):
            assert hip.helper("vlr_gemm_set_sched", mode) == 0
            r.g["C"].copy_(r.c0)
            r.launch(hip)
            torch.cuda.synchronize()
            outs.append(r.g["C"].clone())
    finally:
        torch.cuda.synchronize()
        restore(hip)
    assert not bool(torch.isnan(G.logical(r.inp["C"], outs[0])).any())
    for mode, o in zip((16, 32), outs[1:]):
        assert torch.equal(G.row_bits(outs[0]), G.row_bits(o)), f"sched {mode} differs from sched 0"


# ---------------------------------------------------------------------------------------------------- vlr_gemm_bf16_tn_pair
def _pair_call(hip, p, runs):
    a, b = runs
    hip.call("vlr_gemm_bf16_tn_pair", a.at("A"), a.at("B"), a.at("C"), a.c.M, a.c.N, a.c.lda, a.c.ldb, a.c.ldc,
             b.at("A"), b.at("B"), b.at("C"), b.c.M, b.c.N, b.c.lda, b.c.ldb, b.c.ldc, p.K, p.acc)


@pytest.mark.parametrize("name", [p.name for p in G.PAIRS])
def test_tn_pair(hip, name):
    """the joint launch is ONE gemm_tn bracket of the profiler around ONE gemm256p launch; a fallback is two vlr_gemm_bf16 calls (two
    gemm_tn brackets) and bit-identical to them"""
    p = next(p for p in G.PAIRS if p.name == name)
    runs = [Run(c) for c in p.cases]
    ws = torch.full(((64 << 20) // 4,), NAN, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    try:
        assert hip.helper("vlr_gemm_set_splitk_workspace", ws.data_ptr(), ws.numel() * 4) == 0
        hip.lib_profile_start(1)
        _pair_call(hip, p, runs)
        prof = hip.lib_profile_stop()
        torch.cuda.synchronize()
        first = [r.g["C"].clone() for r in runs]
        wrote_ws = bool((~torch.isnan(ws)).any())
        for r in runs:
            r.g["C"].copy_(r.c0)
        _pair_call(hip, p, runs)
        torch.cuda.synchronize()
        second = [r.g["C"].clone() for r in runs]
        for r in runs:                                                 # the two single calls
            r.g["C"].copy_(r.c0)
            hip.call("vlr_gemm_bf16", 2, r.at("A"), r.at("B"), r.at("C"), None, None, r.c.M, r.c.N, r.c.K, r.c.lda, r.c.ldb, r.c.ldc, 0, 0, p.acc, 0)
        torch.cuda.synchronize()
        single = [r.g["C"].clone() for r in runs]
    finally:
        torch.cuda.synchronize()
        restore(hip)
    n_tn, n256 = prof["gemm_tn"][0], prof["gemm256p"][0]
    assert (n_tn, n256) == ((1, 1) if p.joint else (2, n256)), f"{name}: {n_tn} gemm_tn brackets, {n256} gemm256p launches (joint = {p.joint})"
    assert not wrote_ws, name
    for r, f, s2, sg in zip(runs, first, second, single):
        assert torch.equal(G.row_bits(f), G.row_bits(s2)), f"{r.c.name}: two runs differ"
        if not p.joint:
            assert torch.equal(G.row_bits(f), G.row_bits(sg)), f"{r.c.name}: the fallback differs from the single call"
        for k in ("A", "B"):
            assert torch.equal(G.row_bits(r.g[k].cpu()), G.row_bits(r.inp[k].flat)), f"{r.c.name}: operand {k} was written"
        e = G.expect(r.c, r.inp, DEV if G.macs(r.c) > G.DEVICE_REF_MACS else "cpu")
        G.check(r.c.name, f.cpu(), r.inp["C"], G.Exp(e.ref.cpu(), None, None, None))


# ---------------------------------------------------------------------------------------------------- the register-staged kernel
_CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
from tests import test_hip_gemm_edges as T
T.child_main()
"""


def child_main():
    """every case of the ring subset in THIS process (started with VLR_GEMM128P=0: the register-staged kernel takes what the ring would);
    prints one verdict line"""
    from vlrlhf import _hip
    _hip.lib()
    lines, bad = [], []
    for c in G.RING_SUBSET:
        try:
            run_case(_hip, c, say=lines.append)
        except AssertionError as e:
            bad.append(f"{c.name}: {e}")
    print("\n".join(lines))
    print(f"gemm-edges-child {'FAILED ' + ' | '.join(bad)[:3000] if bad else 'ok'} {len(G.RING_SUBSET)} cases")


def test_ring_subset_on_the_register_staged_kernel(hip):
    """VLR_GEMM128P is read once per process: the whole ring subset again in ONE child process with VLR_GEMM128P=0 (about twenty tiny
    launches; the time limit covers the interpreter's and the library's start-up)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VLR_GEMM128P="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, root, os.path.join(root, "vl-rlhf_amd")], capture_output=True, text=True, timeout=300, env=env,
                       cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    verdict = r.stdout.strip().splitlines()[-1]
    assert verdict == f"gemm-edges-child ok {len(G.RING_SUBSET)} cases", verdict
