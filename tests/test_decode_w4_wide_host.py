"""CPU-only checks of the wide skinny GEMM over packed int4 weights: the header declares the new entry points and the library exports
them (ABI version unchanged), the ctypes signatures are those of the 16-row functions they mirror, the wide scratch size equals the
16-row one up to 16 rows and is M x the per-row size above, argument errors are reported without a GPU, and the engine sizes its decode
scratch for 64-row groups over packed weights exactly when it says it has the wide packed call."""
import os
import re
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vlr_gemv_wide_w4_workspace_bytes", "vlr_gemv_wide_w4", "vlr_gemv_wide_w4_lora"]
SHAPES = [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008), (136, 416), (128, 128), (256, 8192)]      # (N, K)


def header():
    return open(os.path.join(ROOT, "include", "vlr.h")).read()


def prototype_args(hdr, name):
    m = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} has no prototype in include/vlr.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_new_names_are_declared_bound_and_exported():
    from vlrlhf import _hip
    l = _hip.lib()
    hdr = header()
    declared = set(re.findall(r"\b(vlr_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} not declared in include/vlr.h"
        assert hasattr(l, name), f"{name} declared but not exported by libvlr_hip.so"
        assert name in _hip.exported_symbols()
    assert _hip.helper("vlr_abi_version") == 9               # additive entry points: no caller breaks
    fn = l.vlr_gemv_wide_w4_workspace_bytes
    assert fn.restype is _hip.C.c_long and len(fn.argtypes) == prototype_args(hdr, "vlr_gemv_wide_w4_workspace_bytes") == 3
    for wide, narrow in (("vlr_gemv_wide_w4", "vlr_gemv_w4"), ("vlr_gemv_wide_w4_lora", "vlr_gemv_w4_lora")):
        assert _hip._SIGS[wide] == _hip._SIGS[narrow], "the argument list of the 16-row namesake"
        assert len(_hip._SIGS[wide]) == prototype_args(hdr, wide) == prototype_args(hdr, narrow)
        assert list(getattr(l, wide).argtypes) == _hip._SIGS[wide]


def test_wide_w4_scratch_sizes_against_the_16_row_helper():
    from vlrlhf import _hip
    l = _hip.lib()
    for N, K in SHAPES:
        per_row = l.vlr_gemv_w4_workspace_bytes(1, N, K)
        assert per_row > 0
        for M in range(1, 17):
            assert l.vlr_gemv_wide_w4_workspace_bytes(M, N, K) == l.vlr_gemv_w4_workspace_bytes(M, N, K) == M * per_row
        for M in (17, 32, 33, 48, 49, 64):
            assert l.vlr_gemv_wide_w4_workspace_bytes(M, N, K) == M * per_row > l.vlr_gemv_w4_workspace_bytes(M, N, K)      # (that one clamps at 16)
            # the adapter form's sizes are the wide adapter helpers': they cover the packed split count plus the adapter slice
            for rt in (8, 192):
                assert l.vlr_gemv_wide_lora_workspace_bytes(M, N, K, rt) >= l.vlr_gemv_wide_w4_workspace_bytes(M, N, K) + M * N * 4
        assert l.vlr_gemv_wide_w4_workspace_bytes(65, N, K) == l.vlr_gemv_wide_w4_workspace_bytes(64, N, K)
    assert l.vlr_gemv_wide_w4_workspace_bytes(0, 64, 128) == 0 and l.vlr_gemv_wide_w4_workspace_bytes(4, 64, 0) == 0


def test_argument_errors_without_gpu():
    from vlrlhf import _hip
    l = _hip.lib()
    one = 16                                                  # a non-null, 16-byte aligned stand-in pointer: the checks never read it
    #       mode X    ldx  qw   qz   sc   g    Y    ldy bias  res   ldr pos   cos   sin   rc hd   mp M  N   K    ws
    args = [0, one, 128, one, one, one, 128, one, 128, None, None, 0, None, None, None, 0, 128, 0, 4, 64, 128, one]
    for M in (0, 65):
        args[18] = M
        assert l.vlr_gemv_wide_w4(*args, None) == 1
        assert b"vlr_gemv_wide_w4:" in l.vlr_last_error() and b"1 <= M <= 64" in l.vlr_last_error()
        assert l.vlr_gemv_wide_w4_lora(*args, one, one, 8, 1, None, 1.0, one, None) == 1
        assert b"vlr_gemv_wide_w4_lora:" in l.vlr_last_error() and b"1 <= M <= 64" in l.vlr_last_error()
    args[18] = 17
    assert l.vlr_gemv_w4(*args, None) == 1 and b"vlr_gemv_w4:" in l.vlr_last_error() and b"1 <= M <= 16" in l.vlr_last_error()
    assert l.vlr_gemv_w4_lora(*args, one, one, 8, 1, None, 1.0, one, None) == 1 and b"1 <= M <= 16" in l.vlr_last_error()
    args[18] = 40
    assert l.vlr_gemv_wide_w4_lora(*args, one, one, 12, 1, None, 1.0, one, None) == 1 and b"multiple of 8" in l.vlr_last_error()
    args[6] = 48                                             # a group size that is no multiple of 32
    assert l.vlr_gemv_wide_w4(*args, None) == 1 and b"group_size" in l.vlr_last_error()
    args[6], args[19] = 128, 68                              # N % 8 != 0
    assert l.vlr_gemv_wide_w4(*args, None) == 1 and b"multiple of 8" in l.vlr_last_error()


class StubLib:
    """the scratch-size helpers with recognisable values; records the row counts they were asked for"""
    UNITS = {"vlr_gemv_workspace_bytes": 1, "vlr_gemv_w4_workspace_bytes": 2, "vlr_gemv_lora_workspace_bytes": 3, "vlr_gemv_lora_u_bytes": 5,
             "vlr_gemv_wide_workspace_bytes": 7, "vlr_gemv_wide_lora_workspace_bytes": 11, "vlr_gemv_wide_lora_u_bytes": 13,
             "vlr_gemv_wide_w4_workspace_bytes": 17, "vlr_attn_decode_workspace_bytes": 0}

    def __init__(self):
        self.rows = {}

    def __getattr__(self, name):
        unit = self.UNITS.get(name)
        if unit is None:
            raise AttributeError(name)

        def fn(M, *rest):
            self.rows.setdefault(name, set()).add(M)
            return 64 if name == "vlr_attn_decode_workspace_bytes" else 16 * unit * M
        return fn


def decode_ws(monkeypatch, B, lora=None, **attrs):
    import vlrlhf.engine as E
    lib = StubLib()
    monkeypatch.setattr(E._hip, "lib", lambda: lib)
    eng = SimpleNamespace(_ws={}, lora=lora, lora_layout=SimpleNamespace(qkv_targets=3), packed={}, wide_gemv=True, Nqkv=48, H=16, Nq=16,
                          I=32, V=40, nh=1, dev=torch.device("cpu"), RDT=torch.bfloat16, **attrs)
    d = E.LlavaHipEngine._decode_ws(eng, B, 50)
    assert E.LlavaHipEngine._decode_ws(eng, B, 50) is d, "cached per shape"
    assert d["struct"].gemv_ws_bytes == d["gemv"].numel()
    return d, lib.rows


def test_decode_ws_over_packed_weights_is_sized_for_64_row_groups_when_the_engine_has_the_wide_call(monkeypatch):
    from vlrlhf.engine import LlavaHipEngine
    assert LlavaHipEngine.wide_gemv_w4 is True and LlavaHipEngine.wide_gemv is True
    # the engine says it has the wide packed call: min(B, 64) rows of the wide int4 helper (and of the bf16 one, for the lm-head)
    d, rows = decode_ws(monkeypatch, 33, wide_gemv_w4=True)
    assert rows["vlr_gemv_wide_w4_workspace_bytes"] == {33} and rows["vlr_gemv_wide_workspace_bytes"] == {33}
    assert rows["vlr_gemv_w4_workspace_bytes"] == {16} and d["gemv"].numel() == 16 * 17 * 33
    d, rows = decode_ws(monkeypatch, 100, wide_gemv_w4=True)
    assert rows["vlr_gemv_wide_w4_workspace_bytes"] == {64} and d["gemv"].numel() == 16 * 17 * 64
    # live adapters over the packed base: the wide adapter helpers too
    d, rows = decode_ws(monkeypatch, 20, lora={"r": 8}, wide_gemv_w4=True)
    assert rows["vlr_gemv_wide_w4_workspace_bytes"] == rows["vlr_gemv_wide_lora_workspace_bytes"] == rows["vlr_gemv_wide_lora_u_bytes"] == {20}
    assert d["gemv"].numel() == 16 * 17 * 20 and d["u"].numel() == 16 * 13 * 20 == d["lora_struct"].u_bytes
    # up to 16 rows nothing changes
    d, rows = decode_ws(monkeypatch, 16, wide_gemv_w4=True)
    assert d["gemv"].numel() == 16 * 2 * 16 and not any("wide" in k for k in rows)
    # an engine without the attribute (an older subclass, a stub) asks what it asked before: 16-row sizing
    d, rows = decode_ws(monkeypatch, 33)
    assert d["gemv"].numel() == 16 * 2 * 16 and not any("wide" in k for k in rows)
    # so does one that withholds the packed wide call, and wide_gemv = False withholds both
    d, rows = decode_ws(monkeypatch, 33, wide_gemv_w4=False)
    assert d["gemv"].numel() == 16 * 2 * 16 and not any("wide" in k for k in rows)
    import vlrlhf.engine as E
    lib = StubLib()
    monkeypatch.setattr(E._hip, "lib", lambda: lib)
    eng = SimpleNamespace(_ws={}, lora=None, lora_layout=None, packed={}, wide_gemv=False, wide_gemv_w4=True, Nqkv=48, H=16, Nq=16, I=32, V=40, nh=1,
                          dev=torch.device("cpu"), RDT=torch.bfloat16)
    d = E.LlavaHipEngine._decode_ws(eng, 33, 50)
    assert d["gemv"].numel() == 16 * 2 * 16 and not any("wide" in k for k in lib.rows)
