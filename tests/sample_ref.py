"""Host reference (numpy) of include/vlr.h vlr_sample_tokens: the logits-processor chain, the Philox / Gumbel-max draw, the log-prob and the
eos bookkeeping, with the three derived quantities a comparison against the fp32 kernel needs.

Steps 1-3 of the contract (penalty, temperature, top-k) are single correctly rounded fp32 operations and comparisons of exact fp32 values:
numpy fp32 replays them bit for bit.  Steps 4-6 (top-p masses, the Gumbel scores, the log-prob) are computed here in fp64 and compared
within bounds that are formulas of the fp32 unit roundoff U = 2^-24, the kernel's documented reduction depth and the ulp errors of expf /
logf / log1pf (taken as 2 ulp each, i.e. relative 4 U; the device library documents 1 to 2):

  depth(V)   the longest chain of additions behind one of the kernel's sums: 4 * ceil(V / 4096) per thread (its groups in order, 4 columns
             each), 6 butterfly levels, 16 waves, and 17 more where the bisection adds up its slices and what lies above them;
  term       one summand exp(z - m): the subtraction is rounded once (relative U on d = m - z, i.e. relative d U on the exponential) and
             expf adds 4 U: relative (D + 4) U with D = the largest d whose exponential is not yet negligible (min(range, 104));
  eps_p      the kernel keeps a token iff S < fl(top_p * Z), S and Z two such sums: the normalised mass S / Z carries a relative error of
             at most 2 (D + 4 + depth) U + 2 U, and S / Z <= 1, so a kept bit is decidable iff |mass - top_p| >= eps_p;
  delta      a score is s = fl(z + g), g = -logf(E), E = -logf(u) or -log1pf(-(1 - u)) with u exact: E is off by relative 4 U, which moves
             log E by 4 U absolutely, logf adds 4 U |g| with |g| <= 17.33, and the final addition rounds by U |s|:
             err(s) <= (4 + 4 * 17.33) U + U |s|.  Two scores closer than delta = 2 max err(s) cannot be ordered;
  logp       logp = fl(z_tok - fl(m + logf(Zk))): Zk relative (D + 4 + depth) U, which is the absolute error of its logarithm; logf adds
             4 U |log Zk|; the two additions round by U |lse| and U |logp|."""
import numpy as np

from .neftune_ref import philox4x32_10

U = 2.0 ** -24
GUMBEL_MAX = 25 * np.log(2.0)          # -log(-log(1 - 2^-25)) to first order: 17.33


def depth(V):
    return 4 * ((V + 4095) // 4096) + 6 + 16 + 17


def spread(z):
    """D: the largest m - z over the finite entries, capped where expf underflows"""
    f = np.isfinite(z)
    return float(min(104.0, (z[f].max() - z[f].min()) if f.any() else 0.0))


def eps_p(V, D=104.0):
    return (2.0 * (D + 4.0 + depth(V)) + 2.0) * U


def delta(zmax):
    return 2.0 * ((4.0 + 4.0 * GUMBEL_MAX) * U + U * (abs(zmax) + GUMBEL_MAX))


def logp_bound(V, D, logZ, lse, logp):
    return (D + 4.0 + depth(V)) * U + 4.0 * U * abs(logZ) + U * abs(lse) + U * abs(logp) + 1e-12


def history_rows(B, prompt_ids=None, prompt_div=1, gen_ids=None, n_gen=0):
    """per row the ids of its history: all T prompt ids of prompt row r // prompt_div, then the first n_gen generated ones"""
    rows = []
    for r in range(B):
        h = []
        if prompt_ids is not None:
            h += [int(x) for x in np.asarray(prompt_ids)[r // prompt_div]]
        if gen_ids is not None and n_gen:
            h += [int(x) for x in np.asarray(gen_ids)[r][:n_gen]]
        rows.append(h)
    return rows


def warp(logits, hist, penalty, temperature, do_sample, fault=""):
    """steps 1-2 in fp32 -> z [B][V] fp32, bit for bit the kernel's"""
    x = np.array(logits, dtype=np.float32)
    B, V = x.shape
    pen, temp = np.float32(penalty), np.float32(temperature)
    if fault == "pen_after_temp" and do_sample:
        x = x / temp
    if float(pen) != 1.0:
        for r in range(B):
            ids = [i for i in hist[r] if 0 <= i < V]
            for i in (ids if fault == "dup_twice" else sorted(set(ids))):
                x[r, i] = x[r, i] * pen if x[r, i] < 0 else x[r, i] / pen
    if do_sample and fault != "pen_after_temp":
        x = x / temp
    return x + np.float32(0.0)          # -0 -> +0


def gumbel(V, seed, call, step, row_ids, fault=""):
    """fp64 [B][V]: g_i of word i % 4 of the Philox block (i / 4, row_id, step, call), key = the halves of seed"""
    row_ids = np.asarray(row_ids, dtype=np.uint64).reshape(-1, 1)
    blk = np.arange((V + 3) // 4, dtype=np.uint64).reshape(1, -1)
    w = philox4x32_10(blk, row_ids, step, call, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    if fault == "philox_word_shift":
        w = w[1:] + w[:1]
    w = np.stack(w, axis=-1).reshape(row_ids.shape[0], -1)[:, :V]
    r = (w >> np.uint32(8)).astype(np.float64)
    lowhalf = r < 2.0 ** 23
    u_lo = (np.where(lowhalf, r, 0.0) + 0.5) * 2.0 ** -24
    v_hi = (np.where(lowhalf, 0.0, 2.0 ** 24 - 1.0 - r) + 0.5) * 2.0 ** -24
    E = np.where(lowhalf, -np.log(u_lo), -np.log1p(-v_hi))
    return -np.log(E)


def sample_ref(logits, *, do_sample=True, temperature=1.0, top_k=0, top_p=1.0, penalty=1.0, prompt_ids=None, prompt_div=1, gen_ids=None,
               n_gen=0, eos=(), pad=0, seed=0, call=0, step=0, row_ids=None, unfinished=None, finish_step=None, fault=""):
    """-> dict: tok [B] int64, logp [B] fp64, kept [B][V] uint8, unfinished [B] uint8, finish_step [B] int32, and what the checker needs:
    z [B][V] fp32, lse [B], logZ [B], D [B], gap [B] (the two largest perturbed scores' distance), kept_undecidable [B][V] bool.
    fault: a planted deviation, for the checker's own tests only."""
    x = np.asarray(logits, dtype=np.float32)
    B, V = x.shape
    hist = history_rows(B, prompt_ids, prompt_div, gen_ids, n_gen)
    z = warp(x, hist, penalty, temperature, do_sample, fault)
    kept = np.ones((B, V), dtype=bool)
    undec = np.zeros((B, V), dtype=bool)
    Dr = np.array([spread(z[r]) for r in range(B)]) if B <= 4096 else np.full(B, spread(z))
    if do_sample and 0 < top_k < V:
        k = top_k + 1 if fault == "topk_off_by_one" else top_k
        srt = np.sort(z, axis=1)
        kth = srt[:, V - min(k, V)][:, None]
        kept = z >= kth
        if fault == "tie_dropped":      # exactly k survive: the ties with the k-th beyond it are dropped (highest index first)
            order = np.argsort(-z, axis=1, kind="stable")
            kept = np.zeros_like(kept)
            np.put_along_axis(kept, order[:, :k], True, axis=1)
    z64 = z.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if do_sample and np.float32(top_p) < 1:
            tp = float(np.float32(top_p))
            zz = np.where(kept, z64, -np.inf)
            m = zz.max(1, keepdims=True)
            e = np.exp(zz - m)
            p = e / e.sum(1, keepdims=True)
            order = np.argsort(-zz, axis=1, kind="stable")
            ps, zs = np.take_along_axis(p, order, 1), np.take_along_axis(zz, order, 1)
            excl = np.cumsum(ps, 1) - ps
            start = np.ones_like(zs, dtype=bool)
            start[:, 1:] = zs[:, 1:] != zs[:, :-1]
            if fault == "topp_le":      # the inclusive mass compared with <=: the tie group that reaches top_p is lost
                mass_s = np.cumsum(ps, 1)
                keep_s = mass_s <= tp
                keep_s[:, 0] = True
            else:
                mass_s = np.maximum.accumulate(np.where(start, excl, 0.0), axis=1)      # mass of the strictly greater values
                keep_s = mass_s < tp
            mass = np.empty_like(mass_s)
            np.put_along_axis(mass, order, mass_s, axis=1)
            keep_p = np.empty_like(keep_s)
            np.put_along_axis(keep_p, order, keep_s, axis=1)
            undec = kept & (np.abs(mass - tp) < np.array([eps_p(V, d) for d in Dr])[:, None])
            kept = kept & keep_p
        if not do_sample:
            kept = np.ones((B, V), dtype=bool)
        rid = np.arange(B) if (row_ids is None or fault == "rowid_from_position") else np.asarray(row_ids)
        zk = np.where(kept, z64, -np.inf)
        m = zk.max(1)
        Zk = np.exp(zk - m[:, None]).sum(1)
        lse = m + np.log(Zk)
        if fault == "logp_unfiltered":
            mm = z64.max(1)
            lse = mm + np.log(np.exp(z64 - mm[:, None]).sum(1))
        s = zk + gumbel(V, seed, call, step, rid, fault) if do_sample else zk
        tok = s.argmax(1)
        if V > 1:
            top2 = np.partition(s, V - 2, axis=1)[:, V - 2:]
            gap = np.where(np.isfinite(top2[:, 0]), top2[:, 1] - top2[:, 0], np.inf)
        else:
            gap = np.full(B, np.inf)
        if not do_sample:
            gap = np.where(gap == 0, np.inf, gap)      # greedy: an exact tie is decided by the index, and anything else is exact
        logp = z64[np.arange(B), tok] - lse
    unf = np.ones(B, dtype=np.uint8) if unfinished is None else np.array(unfinished, dtype=np.uint8)
    fin = np.full(B, -1, dtype=np.int32) if finish_step is None else np.array(finish_step, dtype=np.int32)
    tok = tok.astype(np.int64)
    done = unf == 0
    if fault != "finished_not_padded":
        tok = np.where(done, pad, tok)
        logp = np.where(done, 0.0, logp)
    hit = np.isin(tok, np.asarray(list(eos), dtype=np.int64)) & ~done
    unf_out = unf.copy()
    if fault != "eos_not_clearing":
        unf_out[hit] = 0
    fin[hit] = step
    return dict(tok=tok, logp=logp, kept=kept.astype(np.uint8), unfinished=unf_out, finish_step=fin, z=z, lse=lse, logZ=np.log(Zk), D=Dr,
                gap=gap, kept_undecidable=undec, done=done, pad=pad, eos=tuple(int(e) for e in eos), step=step, do_sample=do_sample)


def check_sample(out, ref):
    """out: what a candidate produced (dict: tok, logp, unfinished, finish_step, and kept or None) against sample_ref's dict ->
    (fails: list of str, worst logp error / bound, waived: rows whose draw the reference cannot decide).  A row with an undecidable kept
    bit is waived as a whole; a row whose two best scores lie within delta may draw either of them, and its log-prob is then checked at the
    token the candidate drew."""
    fails, worst, waived = [], 0.0, 0
    z, B, V = ref["z"], ref["z"].shape[0], ref["z"].shape[1]
    tok, logp = np.asarray(out["tok"]).astype(np.int64), np.asarray(out["logp"], dtype=np.float64)
    kept = None if out.get("kept") is None else np.asarray(out["kept"])
    zmax = float(np.abs(z[np.isfinite(z)]).max()) if np.isfinite(z).any() else 0.0
    dl = delta(zmax)
    for r in range(B):
        if ref["done"][r]:
            if tok[r] != ref["pad"] or logp[r] != 0.0:
                fails.append(f"row {r}: finished row got token {tok[r]} logp {logp[r]} (pad {ref['pad']}, 0)")
            if out["unfinished"][r] != 0 or out["finish_step"][r] != ref["finish_step"][r]:
                fails.append(f"row {r}: finished row's flags moved")
            continue
        if ref["kept_undecidable"][r].any():
            waived += 1
            continue
        if kept is not None and not np.array_equal(kept[r], ref["kept"][r]):
            bad = np.nonzero(kept[r] != ref["kept"][r])[0]
            fails.append(f"row {r}: kept mask differs at {bad[:8].tolist()} ({bad.size} columns)")
            continue
        t = int(tok[r])
        if not (0 <= t < V) or not ref["kept"][r, t]:
            fails.append(f"row {r}: token {t} outside the kept set")
            continue
        if t != ref["tok"][r]:
            if ref["gap"][r] < dl:
                waived += 1
            else:
                fails.append(f"row {r}: token {t}, reference {ref['tok'][r]} (gap {ref['gap'][r]:.3g} >= delta {dl:.3g})")
                continue
        want = float(z[r, t]) - ref["lse"][r]
        bound = logp_bound(V, ref["D"][r], ref["logZ"][r], ref["lse"][r], want)
        err = abs(logp[r] - want)
        worst = max(worst, err / bound)
        if not err <= bound:
            fails.append(f"row {r}: logp {logp[r]!r}, reference {want!r}: error {err:.3g} > bound {bound:.3g}")
        is_eos = t in ref["eos"]
        if out["unfinished"][r] != (0 if is_eos else 1):
            fails.append(f"row {r}: unfinished {out['unfinished'][r]} after token {t} (eos: {is_eos})")
        want_fin = ref["step"] if is_eos else (ref["finish_step"][r] if t == ref["tok"][r] else None)
        if is_eos and out["finish_step"][r] != ref["step"]:
            fails.append(f"row {r}: finish_step {out['finish_step'][r]}, expected {ref['step']}")
        if not is_eos and want_fin is not None and out["finish_step"][r] != want_fin:
            fails.append(f"row {r}: finish_step moved to {out['finish_step'][r]} without an eos")
    return fails, worst, waived


def chi2_sf(x, df):
    """P(chi-square with df degrees of freedom > x), the closed forms: even df = exp(-x/2) sum_{j < df/2} (x/2)^j / j!, odd df =
    erfc(sqrt(x/2)) + sqrt(2x/pi) exp(-x/2) sum_{j <= (df-3)/2} x^j / (1 * 3 * ... * (2j + 1))"""
    import math
    h = x / 2.0
    if df % 2 == 0:
        term, tot = 1.0, 1.0
        for j in range(1, df // 2):
            term *= h / j
            tot += term
        return math.exp(-h) * tot
    tot, term = 0.0, 1.0
    for j in range((df - 1) // 2):
        term = term * x / (2 * j + 1) if j else 1.0
        tot += term
    return math.erfc(math.sqrt(h)) + math.sqrt(2.0 * x / math.pi) * math.exp(-h) * tot


# ------------------------------------------------------------------------------------------------------------ the kernel tests' inputs
def kernel_cases():
    """the cases of tests/test_hip_sample_kernels.py, as dicts of plain values; make_case() builds the arrays.  The sizes are the smallest
    at which each loop of the kernel can go wrong: one column, one short of / exactly / one past a wave's 64 lanes and the workgroup's 1024
    threads, one past its 4096 columns per sweep, two real vocabularies; ld odd (scalar loads) and a multiple of 4 (16-byte loads)."""
    cases = []
    Vs = [1, 63, 64, 65, 1023, 1024, 1025, 4099]

    def combos(V):
        return [(1.0, 50, 1.0), (0.5, 2, 0.95), (2.0, 0, 0.3), (1.0, V - 1, 0.01), (0.5, V, 1.0), (2.0, V + 1, 0.95), (1.0, 1, 1.0),
                (1.0, 0, 1.0)]
    for i, V in enumerate(Vs):
        for j in (i, (i + 3) % 8, (i + 5) % 8):
            t, k, p = combos(V)[j]
            cases.append(dict(name=f"V{V}-T{t}-k{k}-p{p}", B=3, V=V, ld=V + 5 if j % 2 else (V + 3) // 4 * 4 + 4, temperature=t, top_k=k, top_p=p))
    cases.append(dict(name="B65", B=65, V=1025, ld=1028, temperature=0.5, top_k=50, top_p=0.95))
    cases.append(dict(name="B1", B=1, V=4099, ld=4099, temperature=2.0, top_k=0, top_p=0.3))
    cases.append(dict(name="llava", B=2, V=32000, ld=32000, temperature=1.0, top_k=50, top_p=1.0))
    cases.append(dict(name="qwen-top_p", B=2, V=151936, ld=151944, temperature=1.0, top_k=0, top_p=0.3))
    cases.append(dict(name="ties", B=3, V=1025, ld=1028, temperature=1.0, top_k=50, top_p=0.95, quantum=0.5))
    cases.append(dict(name="ties-k2", B=3, V=65, ld=70, temperature=1.0, top_k=2, top_p=1.0, quantum=2.0))
    cases.append(dict(name="one-finite", B=3, V=65, ld=68, temperature=1.0, top_k=50, top_p=0.3, one_finite=True))
    cases.append(dict(name="greedy", B=3, V=1025, ld=1030, temperature=1.0, top_k=50, top_p=0.3, do_sample=False))
    cases.append(dict(name="greedy-ties", B=3, V=4099, ld=4100, temperature=1.0, top_k=0, top_p=1.0, do_sample=False, quantum=1.0))
    for pen in (1.3, 0.8):
        cases.append(dict(name=f"penalty{pen}", B=6, V=1025, ld=1028, temperature=0.5, top_k=50, top_p=0.95, penalty=pen, T=7, n_gen=5,
                          prompt_div=3))
    cases.append(dict(name="penalty-empty", B=3, V=65, ld=68, temperature=1.0, top_k=0, top_p=1.0, penalty=1.3, T=0, n_gen=0))
    cases.append(dict(name="penalty-greedy-qwen", B=2, V=151936, ld=151936, temperature=1.0, top_k=0, top_p=1.0, penalty=1.005, T=40, n_gen=9,
                      prompt_div=2, do_sample=False))
    for n, c in enumerate(cases):
        c.setdefault("seed", 1000 + n)
    return cases


def make_case(c):
    """-> (kwargs of sample_ref incl. logits [B][V], the reference's dict).  Deterministic: the logits' seed moves on until no kept bit lies
    within eps_p of the top-p cut and no draw within delta of its runner-up (tests/test_sample_checker_host.py asserts both of the result)."""
    B, V = c["B"], c["V"]
    for attempt in range(20):
        rng = np.random.default_rng(c["seed"] + 7919 * attempt)
        x = (rng.standard_normal((B, V)) * 3.0).astype(np.float32)
        if c.get("quantum"):
            x = (np.round(x / c["quantum"]) * c["quantum"]).astype(np.float32)
        if c.get("one_finite"):
            x[0, :] = -np.inf
            x[0, V // 2] = 1.5
        kw = dict(logits=x, do_sample=c.get("do_sample", True), temperature=c["temperature"], top_k=c["top_k"], top_p=c["top_p"],
                  penalty=c.get("penalty", 1.0), seed=0x123456789ABCDEF ^ c["seed"], call=3, step=5 + c["seed"] % 7, pad=0)
        if "T" in c:
            T, n_gen, div = c["T"], c["n_gen"], c.get("prompt_div", 1)
            pr = rng.integers(0, V, size=(B // div, max(T, 1)))[:, :T]
            gen = rng.integers(0, V, size=(B, 16))
            if T >= 4:
                pr[:, 0], pr[:, 1], pr[:, 2] = 0, V - 1, pr[:, 3]           # the ends of the vocabulary, and a duplicate
            if n_gen >= 2:
                gen[:, 1] = gen[:, 0]
                x[np.arange(B), gen[:, 0]] = np.where(np.arange(B) % 2 == 0, 2.5, -2.5).astype(np.float32)      # both signs are penalised
            kw.update(prompt_ids=pr, prompt_div=div, gen_ids=gen, n_gen=n_gen)
        ref = sample_ref(**kw)
        zmax = float(np.abs(ref["z"][np.isfinite(ref["z"])]).max())
        if not ref["kept_undecidable"].any() and not (ref["gap"] < delta(zmax)).any():
            return kw, ref
    raise AssertionError(f"no decidable input for case {c['name']}")
