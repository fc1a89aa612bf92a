"""The LoRA decoder-layer passes of csrc/layers.cpp through the C ABI, gradient by gradient: vlr_decoder_layer_fwd_lora / _bwd_lora,
_fwd_lora_ex / _bwd_lora_ex and _fwd_lora2 / _bwd_lora2 on every case of tests/lora_layer_ref.py against the float64 reference of the
same layer - x_out, the assigned column blocks of u, dx_in, the eight adapter gradients and (base_grads) the six base gradients.
Per tensor err = max|T - ref| / max|ref| must stay within 4 x the bf16 replay's err and the least-squares scale c within
4 x the replay's |c - 1| + 2^-9: the bounds come from the replay (tests/test_lora_layer_checker_host.py shows that it sits under a
quarter of them and that every planted wiring fault exceeds them), never from the kernels.  Every output and scratch buffer starts as
NaN with 4 guard rows behind its M rows, which must stay NaN; each case runs forward, backward, forward, backward and the second
pair must reproduce the first bit for bit; the packed keep masks the forward draws equal the oracle's mask at the offsets of
include/vlr.h, and a case with mask_bits runs a second time with mask_bits = NULL (the hashing route) against the same reference.
Needs a real MI355X: pytest -m gpu"""
import functools

import pytest
import torch

from tests import lora_layer_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
GUARD = 4
BITS_GUARD, BITS_POISON = 64, 0xEE
RESULTS = {}            # (case, route) -> {tensor: (err / bound, |c - 1| / bound, err, c)}


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    _hip.ensure_splitk_workspace(force=True)
    return _hip


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = R.BY_NAME[name]
    inp = R.make(c)
    return c, inp, R.measure(c, inp, inp["ref"], R.replay(c, inp))


def _dev(t, dt=torch.bfloat16):
    return t.to(dt).to(DEV).contiguous()


class Run:
    """one case on the GPU: operands, NaN-poisoned outputs and scratch with their guard rows, the structs of the entry points"""

    def __init__(self, hip, c, inp, use_bits=True):
        from vlrlhf import _hip as HH
        self.hip, self.c, self.inp, self.HH = hip, c, inp, HH
        B, S, M, H, I = c.B, c.S, c.M, c.hidden, c.inter
        self.Nq, self.Nkv = c.heads * R.HEAD_DIM, c.kv_heads * R.HEAD_DIM
        N = self.N = self.Nq + 2 * self.Nkv
        self.two = c.family == "lora2"
        self.Rk = c.r + (c.r_p if self.two else 0)
        res_dt = torch.float32 if c.resid_f32 else torch.bfloat16
        self.w = {k: _dev(inp[k]) for k in ("ln1", "wqkv", "wo", "ln2", "wgu", "wdown")}
        self.w["bqkv"] = _dev(inp["bqkv"]) if c.bias else None
        self.cos = torch.empty(R.MAX_POS, R.HEAD_DIM // 2, device=DEV)
        self.sin = torch.empty_like(self.cos)
        hip.call("vlr_rope_table", self.cos, self.sin, R.MAX_POS, R.HEAD_DIM, R.THETA)
        self.cfg = HH.LlamaCfg(H, I, c.heads, R.HEAD_DIM, R.EPS, R.MAX_POS, self.cos.data_ptr(), self.sin.data_ptr(), c.kv_heads, int(c.resid_f32))
        self.lw = HH.LayerWeights(*(self.w[k].data_ptr() for k in ("ln1", "wqkv", "wo", "ln2", "wgu", "wdown")),
                                  self.w["bqkv"].data_ptr() if c.bias else None)
        self.x_in = _dev(inp["x_in"], res_dt)
        self.dy = _dev(inp["dy"])
        self.pos = inp["pos"].to(torch.int32).to(DEV)
        self.key_mask = inp["key_mask"].to(torch.int32).to(DEV)
        self.rowmask = None if inp["rowmask"] is None else inp["rowmask"].to(torch.uint8).to(DEV)
        Sp = (S + 63) // 64 * 64
        # outputs and scratch: [rows + GUARD][cols], NaN
        shapes = dict(xn1=(M, H), qkv=(M, N), attn=(M, H), x_mid=(M, H), xn2=(M, H), gu=(M, 2 * I), act=(M, I), x_out=(M, H),
                      u=(M, 7 * self.Rk), dact=(M, I), dxn=(M, H), dattn=(M, H), dqkv=(M, N), dx_mid=(M, H), ws_v=(M, 3 * self.Rk),
                      ws_xd=(M, max(H, I)), dx_in=(M, H))
        self.rows = {k: s[0] for k, s in shapes.items()}
        self.buf = {k: torch.empty(s[0] + GUARD, s[1], dtype=res_dt if k in ("x_mid", "x_out") else torch.bfloat16, device=DEV)
                    for k, s in shapes.items()}
        for k in ("rstd1", "rstd2"):
            self.buf[k] = torch.empty(M + GUARD, dtype=torch.float32, device=DEV)
            self.rows[k] = M
        self.lse = torch.zeros(B, c.heads, Sp, dtype=torch.float32, device=DEV)
        self.delta = torch.zeros(B, c.heads, Sp, dtype=torch.float32, device=DEV)
        self.norm_ws = torch.empty(hip.helper("vlr_rmsnorm_bwd_workspace_bytes", H), dtype=torch.uint8, device=DEV)
        self.grad_names = [n for n in R.LORA_GRADS if n in inp["ref"]] + (list(R.BASE_GRADS) if c.base_grads else [])
        for n in self.grad_names:
            rows, cols = (inp["ref"][n].shape + (1,))[:2]
            self.buf[n] = torch.empty(rows + GUARD, cols, dtype=torch.bfloat16, device=DEV)
            self.rows[n] = rows
        self.old = {n: _dev(inp["old"][n]).view(self.rows[n], -1) for n in self.grad_names}
        b = self.buf
        self.acts = HH.LayerActs(*((self.lse if k == "lse" else b[k]).data_ptr()
                                   for k in ("xn1", "rstd1", "qkv", "attn", "lse", "x_mid", "xn2", "rstd2", "gu", "act", "x_out")))
        self.bws = HH.LayerBwdWs(b["dact"].data_ptr(), b["dxn"].data_ptr(), b["dattn"].data_ptr(), b["dqkv"].data_ptr(), b["dx_mid"].data_ptr(),
                                 self.delta.data_ptr(), self.norm_ws.data_ptr())
        self.lg = HH.LoraGrads(*(b[n].data_ptr() if n in b else None for n in (f"d{m}_{g}" for g in R.GROUPS for m in "AB")))
        self.bg = HH.LayerGrads(*(b[n].data_ptr() for n in R.BASE_GRADS)) if c.base_grads else None
        self.bits_bytes = int(hip.lib().vlr_lora_mask_bytes(H, I, M))
        self.sets = [self._adapter(a, use_bits) for a in inp["sets"]]
        self.bc = None
        if self.two:
            bcs = {}
            for g in R.GROUPS:
                if inp["sets"][0]["B_" + g] is None:
                    bcs[g] = None
                    continue
                rows = inp["sets"][0]["B_" + g].shape[0]
                bcs[g] = torch.full((rows + GUARD, self.Rk), NAN, dtype=torch.bfloat16, device=DEV)
                hip.call("vlr_lora_concat_b", self.sets[0]["t"]["B_" + g], c.r, self.sets[1]["t"]["B_" + g], c.r_p, bcs[g], rows)
                torch.cuda.synchronize()
                want = torch.cat([self.sets[0]["t"]["B_" + g], self.sets[1]["t"]["B_" + g]], 1)
                assert torch.equal(bcs[g][:rows], want) and bool(torch.isnan(bcs[g][rows:]).all()), f"vlr_lora_concat_b {g}"
            self.bcs = bcs
            self.bc = HH.LoraBcomb(*(None if bcs[g] is None else bcs[g].data_ptr() for g in R.GROUPS))

    def _adapter(self, a, use_bits):
        c, HH = self.c, self.HH
        t = {k: (None if a[k] is None else _dev(a[k])) for k in (f"{m}_{g}" for g in R.GROUPS for m in "AB")}
        bits = None
        if a["bits"] and use_bits and a["p"] > 0:
            bits = torch.empty(self.bits_bytes + BITS_GUARD, dtype=torch.uint8, device=DEV)
        st = HH.LoraWeights(a["r"], a["scale"], a["p"], *(None if t[k] is None else t[k].data_ptr() for k in (f"{m}_{g}" for g in R.GROUPS for m in "AB")),
                            c.qkv_targets, None if bits is None else bits.data_ptr())
        return dict(t=t, bits=bits, struct=st, a=a)

    def poison(self):
        for k, b in self.buf.items():
            b.fill_(NAN)
            if k in self.old and self.c.accumulate:
                b[:self.rows[k]] = self.old[k]
        for s in self.sets:
            if s["bits"] is not None:
                s["bits"].fill_(BITS_POISON)

    def fwd_bwd(self):
        hip, c, b = self.hip, self.c, self.buf
        self.poison()
        L = self.sets[0]
        if c.family == "lora":
            hip.call("vlr_decoder_layer_fwd_lora", self.cfg, self.lw, L["struct"], self.acts, b["u"], None, L["a"]["seed"], self.x_in, self.pos,
                     self.key_mask, c.B, c.S)
        elif c.family == "lora_ex":
            hip.call("vlr_decoder_layer_fwd_lora_ex", self.cfg, self.lw, L["struct"], self.acts, b["u"], None, L["a"]["seed"], self.rowmask,
                     self.x_in, self.pos, self.key_mask, c.B, c.S)
        else:
            Pw = self.sets[1]
            hip.call("vlr_decoder_layer_fwd_lora2", self.cfg, self.lw, L["struct"], Pw["struct"], self.bc, self.acts, b["u"], L["a"]["seed"],
                     Pw["a"]["seed"], self.rowmask, self.x_in, self.pos, self.key_mask, c.B, c.S)
        torch.cuda.synchronize()
        out = dict(x_out=b["x_out"].clone(), u=b["u"].clone())
        out["bits"] = [None if s["bits"] is None else s["bits"].clone() for s in self.sets]
        if c.family == "lora":
            hip.call("vlr_decoder_layer_bwd_lora", self.cfg, self.lw, L["struct"], self.lg, c.accumulate, self.acts, b["u"], self.bws, b["ws_v"],
                     b["ws_xd"], L["a"]["seed"], self.x_in, self.dy, b["dx_in"], self.pos, self.key_mask, c.B, c.S)
        elif c.family == "lora_ex":
            hip.call("vlr_decoder_layer_bwd_lora_ex", self.cfg, self.lw, self.bg, L["struct"], self.lg, c.accumulate, self.acts, b["u"], self.bws,
                     b["ws_v"], b["ws_xd"], L["a"]["seed"], self.rowmask, self.x_in, self.dy, b["dx_in"], self.pos, self.key_mask, c.B, c.S)
        else:
            Pw = self.sets[1]
            hip.call("vlr_decoder_layer_bwd_lora2", self.cfg, self.lw, L["struct"], self.lg, Pw["struct"], self.bc, c.accumulate, self.acts,
                     b["u"], self.bws, b["ws_v"], L["a"]["seed"], Pw["a"]["seed"], self.rowmask, self.x_in, self.dy, b["dx_in"], self.pos,
                     self.key_mask, c.B, c.S)
        torch.cuda.synchronize()
        for n in ["dx_in"] + self.grad_names:
            out[n] = b[n].clone()
        return out

    def guards_intact(self):
        bad = [k for k, b in self.buf.items() if not bool(torch.isnan(b[self.rows[k]:].float()).all())]
        bad += [f"mask_bits[{i}]" for i, s in enumerate(self.sets)
                if s["bits"] is not None and not bool((s["bits"][self.bits_bytes:] == BITS_POISON).all())]
        return bad

    def host(self, out):
        """the compared tensors on the host, guard rows cut off, shaped as the reference"""
        got = {}
        for n in R.tensors(self.c):
            t = out[n][:self.rows[n]].float().cpu()
            got[n] = t.reshape(self.inp["ref"][n].shape)
        return got


def _same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, list):
        return all(_same_bits(x, y) for x, y in zip(a, b))
    iv = {2: torch.int16, 4: torch.int32, 1: torch.uint8}[a.element_size()]
    return torch.equal(a.view(iv), b.view(iv))


def _check(hip, c, inp, replay_meas, use_bits):
    route = "bits" if use_bits and (c.mask_bits or c.mask_bits_p) else "hash" if (c.dropout > 0 or c.dropout_p > 0) else "p0"
    run = Run(hip, c, inp, use_bits)
    first = run.fwd_bwd()
    bad = run.guards_intact()
    assert not bad, f"{c.name}: guard rows written: {bad}"
    second = run.fwd_bwd()
    diff = [k for k in first if not _same_bits(first[k], second[k])]
    assert not diff, f"{c.name}: the second forward / backward differs in {diff}"
    assert not run.guards_intact()
    # the packed keep masks the forward drew: the oracle's mask, LSB first, at the offsets of include/vlr.h
    for s, bits in zip(run.sets, first["bits"]):
        if bits is None:
            continue
        for g in R.GROUPS:
            n, inn, _ = R._group_shape(c, g)
            if s["t"]["A_" + g] is None:
                continue
            for i in range(n):
                o0, nb = R.bits_offset(c, R.T0[g] + i), c.M * inn // 8
                assert torch.equal(bits[o0:o0 + nb].cpu(), R.packed_bits(s["a"], R.T0[g] + i, c.M, inn)), (c.name, g, i)
    got = run.host(first)
    ref = inp["ref"]
    # unmarked rows of a row-restricted adapter's u are zero, exactly
    if inp["rowmask"] is not None:
        um = got["u"].view(c.M, 7, run.Rk)[:, :, (c.r if run.two else 0):]
        rm = ref["u"].view(c.M, 7, run.Rk)[:, :, (c.r if run.two else 0):]
        text = ~inp["rowmask"]
        assert float(um[text][~torch.isnan(rm[text])].abs().max() if text.any() else 0.0) == 0.0, f"{c.name}: u is not zero on the text rows"
    meas = R.measure(c, inp, ref, got)
    rat = R.ratios(meas, replay_meas)
    RESULTS[(c.name, route)] = {n: rat[n] + meas[n] for n in rat}
    for n in rat:
        print(f"  {c.name:48s} {route:4s} {n:8s} err {meas[n][0]:.3e} (replay {replay_meas[n][0]:.3e}) c-1 {meas[n][1] - 1:+.3e} "
              f"(replay {replay_meas[n][1] - 1:+.3e})  err/bound {rat[n][0]:.3f}  |c-1|/bound {rat[n][1]:.3f}")
    over = {n: v for n, v in rat.items() if not (v[0] <= 1.0 and v[1] <= 1.0)}
    assert not over, f"{c.name} [{route}]: over the bound (err / bound, |c - 1| / bound): {over}"
    if c.rowmask == "zero" and c.family == "lora_ex" and not c.base_grads and not c.accumulate:
        assert all(float(got[n].abs().max()) == 0.0 for n in R.LORA_GRADS if n in got), f"{c.name}: dA / dB are not exactly zero"


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_lora_layer_passes_vs_float64(hip, name):
    c, inp, replay_meas = _inputs(name)
    _check(hip, c, inp, replay_meas, True)


@pytest.mark.parametrize("name", [c.name for c in R.CASES if c.mask_bits or c.mask_bits_p])
def test_lora_layer_passes_hashing_route(hip, name):
    """the cases that carry packed masks, with mask_bits = NULL: every kernel hashes; same reference, same bounds"""
    c, inp, replay_meas = _inputs(name)
    _check(hip, c, inp, replay_meas, False)


def test_worst_ratios_per_family():
    """the table of profiles/lora_layer_parity.txt: the worst err / bound and |c - 1| / bound per family over the cases that ran"""
    if not RESULTS:
        return
    print("\nfamily   worst err/bound (case, route, tensor)   worst |c-1|/bound (case, route, tensor)")
    for fam in ("lora", "lora_ex", "lora2"):
        rows = [(v[0], v[1], name, route, n) for (name, route), d in RESULTS.items() if R.BY_NAME[name].family == fam for n, v in d.items()]
        if not rows:
            continue
        we, wc = max(rows, key=lambda t: t[0]), max(rows, key=lambda t: t[1])
        print(f"{fam:8s} {we[0]:.3f} ({we[2]}, {we[3]}, {we[4]})   {wc[1]:.3f} ({wc[2]}, {wc[3]}, {wc[4]})")
        assert we[0] <= 1.0 and wc[1] <= 1.0
