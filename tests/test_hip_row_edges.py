"""Row, reduction, loss and optimizer kernels (csrc/elementwise.hip, csrc/dpo_ops.hip) at their loop edges: every case of tests/row_ref.py
through the C ABI against the float64 / exact reference, element by element, outputs pre-filled with NaN (integer outputs: a sentinel)
and checked for writes beside the result.  tests/test_row_checker_host.py runs the same checkers on the CPU.  Needs a real MI355X:
pytest -m gpu"""
import pytest
import torch

from tests import row_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlrlhf import _hip
    _hip.lib()
    return _hip


def params(*ops):
    ps = R.all_cases(ops)
    return pytest.mark.parametrize("p", ps, ids=[R.case_id(p) for p in ps])


def workspace(nbytes):
    return torch.full((max(nbytes // 4, 1),), float("nan"), dtype=torch.float32, device=DEV)      # no kernel may rely on a zeroed workspace


class Run:
    """one case on the GPU: the inputs (d), the poisoned output buffers (g) and views at their logical start (o)"""

    def __init__(self, p, inp=None):
        self.op, self.c = R.OPS[p[0]], p[1]
        self.inp = self.op.make(self.c) if inp is None else inp
        self.d = {k: v.to(DEV) if isinstance(v, torch.Tensor) else v for k, v in self.inp.items()}
        self.bufs = self.op.buffers(self.c, self.inp)
        self.g = {k: b.flat.to(DEV) for k, b in self.bufs.items()}
        self.o = {k: self.g[k][b.off:] for k, b in self.bufs.items()}

    def out(self, k):
        return self.o.get(k)

    def check(self, only=None):
        torch.cuda.synchronize()
        exp = R.expect(self.op, self.c, self.inp)
        assert set(exp) <= set(self.bufs)
        for k, e in exp.items():
            if only is not None and k not in only:
                continue
            after = self.g[k].cpu()
            what = f"{self.op.name} {self.c.name} {k}"
            if e.rel is not None:
                print(f"{what}: worst |error| / bound = {R.worst_ratio(after, self.bufs[k], e):.3f}")
            R.check(what, after, self.bufs[k], e)
        return exp


# ---------------------------------------------------------------------------------------------------- norms
@params("rmsnorm_fwd", "rmsnorm_fwd_f32")
def test_rmsnorm_fwd(hip, p):
    r = Run(p)
    c, d, o = r.c, r.d, r.o
    hip.call("vlr_" + r.op.name, d["x"], d["w"], o["y"], o["rstd"], c.M, c.H, d["eps"])
    r.check()


@params("rmsnorm_bwd", "rmsnorm_bwd_f32")
def test_rmsnorm_bwd(hip, p):
    r = Run(p)
    c, d, o = r.c, r.d, r.o
    ws = workspace(hip.helper("vlr_rmsnorm_bwd_workspace_bytes", c.H))
    hip.call("vlr_" + r.op.name, d["dy"], d["x"], d["w"], d["rstd"], d["dres"], o["dx"], r.out("dw"), c.acc, ws, c.M, c.H)
    r.check()


@pytest.mark.parametrize("name", ["vlr_rmsnorm_bwd", "vlr_rmsnorm_bwd_f32"])
def test_rmsnorm_bwd_refuses_rows_wider_than_its_registers(hip, name):
    M, H = 2, 8200
    x = torch.zeros(M, H, dtype=torch.float32 if name.endswith("f32") else torch.bfloat16, device=DEV)
    b = torch.zeros(M, H, dtype=torch.bfloat16, device=DEV)
    ws = workspace(hip.helper("vlr_rmsnorm_bwd_workspace_bytes", H))
    with pytest.raises(ValueError):
        hip.call(name, b, x, b[0], torch.ones(M, device=DEV), None, torch.empty_like(b), torch.empty_like(b[0]), 0, ws, M, H)


@params("layernorm_fwd")
def test_layernorm_fwd(hip, p):
    r = Run(p)
    c, d, o = r.c, r.d, r.o
    hip.call("vlr_layernorm_fwd", d["x"], d["w"], d["b"], o["y"], c.M, c.D, d["eps"])
    r.check()


@params("vit_embed_ln")
def test_vit_embed_ln(hip, p):
    r = Run(p)
    c, d, o = r.c, r.d, r.o
    hip.call("vlr_vit_embed_ln", d["pe"], d["cls"], d["pos"], d["w"], d["b"], o["y"], c.n_img, c.T, c.D, d["eps"])
    r.check()


def test_layernorm_fwd_refuses_rows_wider_than_its_registers(hip):
    D = 4104
    x = torch.zeros(6, D, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError):
        hip.call("vlr_layernorm_fwd", x, x[0], x[0], torch.empty_like(x), 6, D, 1e-5)
    with pytest.raises(ValueError):
        hip.call("vlr_vit_embed_ln", x[:4], x[0], x[:3], x[0], x[0], torch.empty_like(x), 2, 3, D, 1e-5)


@params("layernorm_bwd")
def test_layernorm_bwd(hip, p):
    r = Run(p)
    c, d = r.c, r.d
    ws = workspace(hip.helper("vlr_layernorm_bwd_workspace_bytes", c.D))
    hip.call("vlr_layernorm_bwd", d["dy"], d["x"], d["w"], d["eps"], r.out("dx"), r.out("dw"), r.out("db"), c.acc, ws, c.M, c.D)
    r.check()


# ---------------------------------------------------------------------------------------------------- reductions
@params("colsum", "colsum_f32")
def test_colsum(hip, p):
    r = Run(p)
    c, d, o = r.c, r.d, r.o
    X = d["flat"][8 + c.off:]
    assert X.data_ptr() % 16 == (8 if c.off else 0)
    ws = workspace(hip.helper("vlr_colsum_workspace_bytes", c.C))
    if r.op.f32:
        hip.call("vlr_colsum_f32", X, c.R, c.C, c.ld, o["out"], ws)
    else:
        hip.call("vlr_colsum", X, c.R, c.C, c.ld, o["out"], c.acc, ws)
    r.check()


@params("rowdot")
def test_rowdot(hip, p):
    r = Run(p)
    hip.call("vlr_rowdot", r.d["X"], r.d["v"], r.o["out"], r.c.M, r.c.H)
    r.check()


@params("seq_sum")
def test_seq_sum(hip, p):
    r = Run(p)
    hip.call("vlr_seq_sum", r.d["tok"], r.d["seq_off"], len(r.c.lens), r.c.avg, r.o["out"])
    r.check()


# ---------------------------------------------------------------------------------------------------- elementwise, grid-stride
@params("swiglu_fwd")
def test_swiglu_fwd(hip, p):
    r = Run(p)
    hip.call("vlr_swiglu_fwd", r.d["gu"], r.o["act"], r.c.M, r.c.I)
    r.check()


@params("swiglu_bwd")
def test_swiglu_bwd(hip, p):
    r = Run(p)
    hip.call("vlr_swiglu_bwd", r.o["gu"], r.d["dact"], r.c.M, r.c.I)      # in place on [gate | up]
    r.check()


@params("gelu_fwd")
def test_gelu_fwd(hip, p):
    r = Run(p)
    hip.call("vlr_gelu_fwd", r.d["z"], r.o["h"], r.c.n)
    r.check()


@params("gelu_bwd")
def test_gelu_bwd(hip, p):
    r = Run(p)
    hip.call("vlr_gelu_bwd", r.d["z"], r.d["dh"], r.o["dz"], r.c.n)
    r.check()


@params("dropout")
def test_dropout(hip, p):
    """EVERY element against the oracle's hash (row_ref.Dropout.make: oracle dropout_mask): the head, the tail and the window across
    the grid-stride seam are part of it"""
    r = Run(p)
    c = r.c
    hip.call("vlr_dropout", r.d["x"], r.o["out"], c.n, c.p, c.seed, c.alpha, c.add)
    r.check()


@params("dropout_mask")
def test_dropout_mask(hip, p):
    r = Run(p)
    hip.call("vlr_dropout_mask", r.o["mask"], r.c.n, r.c.p, r.c.seed)
    r.check()


@params("dropout_bits")
def test_dropout_bits(hip, p):
    r = Run(p)
    c = r.c
    hip.call("vlr_dropout_bits", r.o["bits"], c.n, c.p, c.seed)
    r.check()
    mask = torch.full((c.n,), 0xA5, dtype=torch.uint8, device=DEV)
    hip.call("vlr_dropout_mask", mask, c.n, c.p, c.seed)       # the packed form of the byte mask, everywhere
    torch.cuda.synchronize()
    bits = R.logical(r.bufs["bits"], r.g["bits"].cpu()).reshape(-1)
    assert torch.equal(bits, R.pack_bits(mask.cpu()))


@params("im2col")
def test_im2col(hip, p):
    r = Run(p)
    c = r.c
    hip.call("vlr_im2col", r.d["px"], r.o["out"], c.n, c.S, c.P, c.Kp)
    r.check()


@params("cast_f32_to_bf16", "cast_bf16_to_f32")
def test_casts(hip, p):
    r = Run(p)
    hip.call("vlr_" + r.op.name, r.d["src"], r.o["dst"], r.c.n)
    r.check()


# ---------------------------------------------------------------------------------------------------- copies
@params("gather_rows")
def test_gather_rows(hip, p):
    r = Run(p)
    hip.call("vlr_gather_rows", r.d["src"], r.d["rows"], r.o["dst"], r.c.R, r.c.H)
    r.check()


@params("scatter_rows")
def test_scatter_rows(hip, p):
    r = Run(p)
    hip.call("vlr_scatter_rows", r.d["src"], r.d["rows"], r.o["dst"], r.c.R, r.c.H)
    r.check()


@params("rows_gather")
def test_rows_gather(hip, p):
    r = Run(p)
    hip.call("vlr_rows_gather", r.d["src"], r.c.lds, r.d["rows"], r.o["dst"], r.c.R, r.c.W)
    r.check()


@params("rows_add")
def test_rows_add(hip, p):
    r = Run(p)
    hip.call("vlr_rows_add", r.d["src"], r.d["rows"], r.o["dst"], r.c.ldd, r.c.R, r.c.W)
    r.check()


@params("merge_fwd_f32")
def test_merge_fwd_f32(hip, p):
    op, c = R.OPS[p[0]], p[1]
    inp = op.make(c)
    Bn, T, S, P = c.Bn, c.T, inp["S"], c.P
    nf = inp["feats"].shape[0]
    src = torch.full((Bn, S), -7777777, dtype=torch.int32, device=DEV)
    omask, opos = torch.empty_like(src), torch.empty_like(src)
    olab = torch.empty(Bn, S, dtype=torch.int64, device=DEV)
    imap = torch.empty(Bn, S, dtype=torch.uint8, device=DEV)
    inv = torch.empty(2, nf, dtype=torch.int32, device=DEV)
    info = torch.zeros(2, dtype=torch.int32, device=DEV)
    ids = inp["ids"].to(DEV)
    hip.call("vlr_merge_index", ids, inp["am"].to(DEV), inp["lab"].to(DEV), Bn, T, S, P, inp["image_token"], inp["model_pad"], nf, 2,
             src, omask, olab, opos, imap, inv, info)
    torch.cuda.synchronize()
    assert torch.equal(src.cpu(), op.cpu_src(c, inp))
    assert int((src == op.SRC_ZERO).sum()) > 0                 # padded rows: exactly zero in the output
    inp["src"] = src.cpu()
    r = Run(p, inp)
    hip.call("vlr_merge_fwd_f32", src, ids, r.d["table"], r.d["feats"], c.feats_f32, r.o["out"], Bn, T, S, c.H)
    r.check()
    out = R.logical(r.bufs["out"], r.g["out"].cpu())
    assert float(out[(inp["src"].reshape(-1) == op.SRC_ZERO)].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------- rope
@params("rope_heads")
def test_rope_heads(hip, p):
    r = Run(p)
    c, d = r.c, r.d
    hip.call("vlr_rope_heads", r.o["qkv"], d["pos"], d["cos"], d["sin"], c.M, c.nh, c.hd, c.ld, c.max_pos, c.bwd)
    r.check()


@pytest.mark.parametrize("hd", [16, 64, 128])
def test_rope_forward_then_backward_restores_the_input(hip, hd):
    """within two bf16 roundings: the forward's (2^-8 of the rotated value, carried back through the rotation: |o1| + |o2| bounds it)
    and the backward's (2^-8 of the restored value), plus the fp32 arithmetic of both"""
    op = R.OPS["rope_heads"]
    c = next(c for c in op.cases if c.hd == hd and not c.bwd)
    r = Run(("rope_heads", c))
    d = r.d
    for bwd in (0, 1):
        hip.call("vlr_rope_heads", r.o["qkv"], d["pos"], d["cos"], d["sin"], c.M, c.nh, c.hd, c.ld, c.max_pos, bwd)
    torch.cuda.synchronize()
    fwd = op.formula(c, r.inp, R.F64)["qkv"][0].reshape(c.M, c.nh, 2, hd // 2)
    x = r.inp["qkv"][:, :c.nh * hd].double()
    carried = (fwd.abs().sum(2, keepdim=True).expand_as(fwd)).reshape(c.M, c.nh * hd)
    # |x_i| <= |o1| + |o2| (a rotation): 2^-10 of the carried term covers the fp32 arithmetic of both calls
    e = R.Exp(x, carried, R.U_BF16, R.U_BF16 * (1 + 2.0 ** -10))
    after = r.g["qkv"].cpu()
    print(f"rope roundtrip hd{hd}: worst |error| / bound = {R.worst_ratio(after, r.bufs['qkv'], e):.3f}")
    R.check(f"rope roundtrip hd{hd}", after, r.bufs["qkv"], e)


# ---------------------------------------------------------------------------------------------------- logps
@params("build_rows")
def test_build_rows(hip, p):
    r = Run(p)
    c, d, o = r.c, r.d, r.o
    hip.call("vlr_build_rows", d["labels"], d["shared"], c.Bn, c.S, -100, o["rows"], o["tgt"], o["seq_off"])
    r.check()


@params("logp_rows")
def test_logp_rows(hip, p):
    r = Run(p)
    c, d, o = r.c, r.d, r.o
    hip.call("vlr_logp_rows", d["logits"], d["row_idx"], d["tgt"], c.R, c.V, c.ld, o["tok"], o["lse"])
    r.check()


@params("dlogits_rows")
def test_dlogits_rows(hip, p):
    r = Run(p)
    c, d, o = r.c, r.d, r.o
    hip.call("vlr_dlogits_rows", d["logits"], d["tgt"], d["lse"], d["seq_off"], len(r.op.LENS), d["dlogps"], c.avg, c.R, c.V, c.ld, o["dl"], c.ldd)
    r.check()


# ---------------------------------------------------------------------------------------------------- loss
@params("dpo_loss")
def test_dpo_loss(hip, p):
    r = Run(p)
    c, d, o = r.c, r.d, r.o
    hip.call("vlr_dpo_loss", d["pc"], d["pr"], d["rc"], d["rr"], c.n, r.op.BETA, c.ls, R.LOSS_IDS[c.lt], c.rf, o["losses"], o["cr"], o["rr"],
             o["dpc"], o["dpr"], o["mean"], d["up"])
    torch.cuda.synchronize()
    for k in r.g:
        assert bool(torch.isfinite(R.logical(r.bufs[k], r.g[k].cpu())).all()), k
    r.check()


def test_dpo_loss_refuses_more_pairs_than_one_workgroup(hip):
    t = torch.zeros(2 * 1025, device=DEV)
    with pytest.raises(ValueError):
        hip.call("vlr_dpo_loss", t, t, t, t, 1025, 0.1, 0.0, 0, 0, t, t, t, t, t, t, None)


# ---------------------------------------------------------------------------------------------------- optimizer
@params("grad_sqnorm")
def test_grad_sqnorm(hip, p):
    r = Run(p)
    c = r.c
    ws = workspace(hip.helper("vlr_grad_sqnorm_workspace_bytes"))
    hip.call("vlr_grad_sqnorm", r.d["g"], 8 * c.n8, c.max_norm, c.gscale, c.extra, ws, r.o["out3"])
    r.check()


@params("adamw_step")
def test_adamw_step(hip, p):
    op, c = R.OPS[p[0]], p[1]
    coef, out3 = None, None
    if c.coef:                                                  # the out3 of a clipping vlr_grad_sqnorm over the same gradient
        sq = R.OPS["grad_sqnorm"]
        cc = R.Case(name="clip", n8=c.n8, gscale=1.0, extra=0.0, max_norm=0.01)
        rs = Run(("grad_sqnorm", cc), dict(g=op.make(c, coef=1.0)["g"]))
        ws = workspace(hip.helper("vlr_grad_sqnorm_workspace_bytes"))
        hip.call("vlr_grad_sqnorm", rs.d["g"], 8 * c.n8, cc.max_norm, cc.gscale, cc.extra, ws, rs.o["out3"])
        rs.check()
        out3 = rs.o["out3"]
        coef = float(out3[1])
        assert coef < 1.0
    r = Run(p, op.make(c, coef=coef))
    d, o, hp = r.d, r.o, op.HP
    hip.call("vlr_adamw_step", o["master"], o["m"], o["v"], d["g"], o["p16"], 8 * c.n8, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], c.wd, c.step, out3)
    r.check()
    master = R.logical(r.bufs["master"], r.g["master"].cpu())
    R.check(f"adamw_step {c.name} p16", r.g["p16"].cpu(), r.bufs["p16"], R.Exp(master.bfloat16(), None, None, None))
