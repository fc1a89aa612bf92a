"""The run-time switches of the package are the ones INTEGRATION.md lists, no more and no fewer.

Every `VLR_*` environment variable read under vl-rlhf_amd/ (csrc/: through vlr_env_int / vlr_env_str / vlr_diag_env_int of common.h,
vlrlhf/: through os.environ) must stand in one of the two tables of INTEGRATION.md - switches of the product library, switches of a
diagnostics build - and every row of the tables must be read somewhere.  In csrc/ a name is decoded at ONE place, so that two readers
cannot disagree about what a value means, and nothing reads the environment behind the helpers' back."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vl-rlhf_amd")
MAX_PRODUCT_SWITCHES = 20      # VERDICT.md, "Next round" item 5

C_PRODUCT = re.compile(r'\bvlr_env_(?:int|str)\(\s*"(VLR_\w+)"')
C_DIAG = re.compile(r'\bvlr_diag_env_int\(\s*"(VLR_\w+)"')
C_RAW = re.compile(r'\b(?:secure_)?getenv\(\s*"(\w+)"')
PY_READ = re.compile(r'''(?:environ(?:\.get|\.setdefault|\.pop)?|getenv)\s*[\[(]\s*["'](VLR_\w+)["']''')


def _files(sub, exts):
    for d, _, names in os.walk(os.path.join(PKG, sub)):
        if os.path.basename(d).startswith("build") or "__pycache__" in d:
            continue
        for n in sorted(names):
            if n.endswith(exts):
                yield os.path.join(d, n)


def _csrc_reads():
    product, diag, raw = [], [], []
    for path in _files("csrc", (".h", ".hip", ".cpp")):
        text = open(path).read()
        where = os.path.basename(path)
        product += [(m, where) for m in C_PRODUCT.findall(text)]
        diag += [(m, where) for m in C_DIAG.findall(text)]
        raw += [(m, where) for m in C_RAW.findall(text)]
    return product, diag, raw


def _python_reads():
    names = set()
    for path in list(_files("vlrlhf", (".py",))) + [os.path.join(PKG, "build_hip.py")]:
        names.update(PY_READ.findall(open(path).read()))
    return names


def _tables():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    a = text.index("### Switches of the product library")
    b = text.index("### Switches of a diagnostics build only")
    end = text.index("\n\n", text.index("\n|", b))          # the diagnostics table ends at the first blank line behind its rows

    def rows(part):
        out = []
        for line in part.split("\n"):
            if line.startswith("| `VLR_"):
                out += re.findall(r"`(VLR_\w+)`", line.split("|")[1])
        return out
    return rows(text[a:b]), rows(text[b:end])


def test_switch_table_matches_the_source():
    product, diag, raw = _csrc_reads()
    assert not raw, f"csrc/ reads the environment without vlr_env_int / vlr_env_str / vlr_diag_env_int (common.h): {raw}"
    for kind, reads in (("vlr_env_*", product), ("vlr_diag_env_int", diag)):
        names = [n for n, _ in reads]
        twice = sorted({n for n in names if names.count(n) > 1})
        assert not twice, f"decoded at more than one place in csrc/ ({kind}): {[(n, w) for n, w in reads if n in twice]}"
    both = {n for n, _ in product} & {n for n, _ in diag}
    assert not both, f"read as a product switch and as a diagnostics switch: {sorted(both)}"

    t_product, t_diag = _tables()
    assert len(t_product) == len(set(t_product)) and len(t_diag) == len(set(t_diag)), "a switch is listed twice in INTEGRATION.md"
    read_product = {n for n, _ in product} | _python_reads()
    read_diag = {n for n, _ in diag}
    assert read_product == set(t_product), (f"read but not in the product table: {sorted(read_product - set(t_product))}; "
                                            f"in the table but read nowhere: {sorted(set(t_product) - read_product)}")
    assert read_diag == set(t_diag), (f"read but not in the diagnostics table: {sorted(read_diag - set(t_diag))}; "
                                      f"in the table but read nowhere: {sorted(set(t_diag) - read_diag)}")
    assert len(t_product) <= MAX_PRODUCT_SWITCHES, f"{len(t_product)} product switches; at most {MAX_PRODUCT_SWITCHES} may remain"


def test_diagnostics_switches_are_compiled_out_of_the_product():
    """a vlr_diag_env_int call stands between an #ifdef / #if of a build define and its #endif"""
    for path in _files("csrc", (".hip", ".cpp")):
        depth = 0
        for i, line in enumerate(open(path).read().split("\n"), 1):
            s = line.strip()
            if re.match(r"#\s*if", s):
                depth += 1
            elif re.match(r"#\s*endif", s):
                depth -= 1
            elif C_DIAG.search(line):
                assert depth > 0, f"{os.path.basename(path)}:{i}: a diagnostics switch is read by the product build"
