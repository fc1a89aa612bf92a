"""CPU-only checks of the wide skinny GEMM and of chunked PPO sampling: the header declares the new entry points and the library
exports them (ABI version unchanged), the ctypes signatures match, the wide scratch sizes dominate the 16-row ones and equal them up
to 16 rows, argument errors are reported without a GPU, the engine sizes its decode scratch for 64-row groups exactly when the wide
path can run, and VLPPOTrainer.generate(batch_size=k) samples the queries k at a time, in order."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vlr_gemv_wide_workspace_bytes", "vlr_gemv_wide_lora_workspace_bytes", "vlr_gemv_wide_lora_u_bytes", "vlr_gemv_wide_bf16",
       "vlr_gemv_wide_bf16_lora"]
SHAPES = [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008), (151936, 4096), (72, 136), (64, 1024)]      # (N, K)


def header():
    return open(os.path.join(ROOT, "include", "vlr.h")).read()


def prototype_args(hdr, name):
    m = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} has no prototype in include/vlr.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_export_list_and_signatures_agree():
    from vlrlhf import _hip
    l = _hip.lib()
    hdr = header()
    declared = set(re.findall(r"\b(vlr_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} not declared in include/vlr.h"
        assert hasattr(l, name), f"{name} declared but not exported by libvlr_hip.so"
        assert name in _hip.exported_symbols()
    assert _hip.helper("vlr_abi_version") == 9               # additive entry points: no caller breaks
    for name in NEW[:3]:
        fn = getattr(l, name)
        assert fn.restype is _hip.C.c_long and len(fn.argtypes) == prototype_args(hdr, name)
    for wide, narrow in (("vlr_gemv_wide_bf16", "vlr_gemv_bf16"), ("vlr_gemv_wide_bf16_lora", "vlr_gemv_bf16_lora")):
        assert _hip._SIGS[wide] == _hip._SIGS[narrow], "the argument list of the 16-row namesake"
        assert len(_hip._SIGS[wide]) == prototype_args(hdr, wide) and list(getattr(l, wide).argtypes) == _hip._SIGS[wide]
    assert [f for f, _ in _hip.DecodeWs._fields_] == ["xn", "rstd", "qkv", "attn", "act", "gemv_ws", "gemv_ws_bytes", "attn_ws", "attn_ws_bytes"]


def test_wide_scratch_sizes_against_the_16_row_helpers():
    from vlrlhf import _hip
    l = _hip.lib()
    for N, K in SHAPES:
        for rt in (8, 192, 792):
            for M in range(1, 17):
                assert l.vlr_gemv_wide_workspace_bytes(M, N, K) == l.vlr_gemv_workspace_bytes(M, N, K) > 0
                assert l.vlr_gemv_wide_lora_workspace_bytes(M, N, K, rt) == l.vlr_gemv_lora_workspace_bytes(M, N, K, rt) > 0
                assert l.vlr_gemv_wide_lora_u_bytes(M, K, rt) == l.vlr_gemv_lora_u_bytes(M, K, rt) > 0
            for M in (17, 32, 33, 64):
                per_row = l.vlr_gemv_workspace_bytes(1, N, K)
                assert l.vlr_gemv_wide_workspace_bytes(M, N, K) == M * per_row > l.vlr_gemv_workspace_bytes(M, N, K)      # (that one clamps at 16)
                assert l.vlr_gemv_wide_lora_workspace_bytes(M, N, K, rt) == M * l.vlr_gemv_lora_workspace_bytes(1, N, K, rt)
                assert l.vlr_gemv_wide_lora_u_bytes(M, K, rt) == l.vlr_gemv_wide_workspace_bytes(M, rt, K) >= l.vlr_gemv_lora_u_bytes(M, K, rt)
            assert l.vlr_gemv_wide_workspace_bytes(65, N, K) == l.vlr_gemv_wide_workspace_bytes(64, N, K)
    assert l.vlr_gemv_wide_workspace_bytes(0, 64, 128) == 0 and l.vlr_gemv_wide_lora_workspace_bytes(4, 64, 128, 12) == 0


def test_argument_errors_without_gpu():
    from vlrlhf import _hip
    l = _hip.lib()
    one = 16                                                  # a non-null, 16-byte aligned stand-in pointer: the checks never read it
    args = [0, one, 128, one, one, 64, None, None, 0, None, None, None, 0, 128, 0, 4, 64, 128, one]
    for M in (0, 65):
        args[15] = M
        assert l.vlr_gemv_wide_bf16(*args, None) == 1
        assert b"vlr_gemv_wide_bf16" in l.vlr_last_error() and b"1 <= M <= 64" in l.vlr_last_error()
        assert l.vlr_gemv_wide_bf16_lora(*args, one, one, 8, 1, None, 1.0, one, None) == 1
        assert b"vlr_gemv_wide_bf16_lora" in l.vlr_last_error() and b"1 <= M <= 64" in l.vlr_last_error()
    args[15] = 17
    assert l.vlr_gemv_bf16(*args, None) == 1 and b"1 <= M <= 16" in l.vlr_last_error()
    args[15] = 40
    assert l.vlr_gemv_wide_bf16_lora(*args, one, one, 12, 1, None, 1.0, one, None) == 1 and b"multiple of 8" in l.vlr_last_error()
    args[16] = 128                                           # K = 128 < ldx is fine; K % 8 != 0 is not
    args[17] = 124
    assert l.vlr_gemv_wide_bf16(*args, None) == 1 and b"multiple of 8" in l.vlr_last_error()


class StubLib:
    """the scratch-size helpers with recognisable values; records the row counts they were asked for"""

    def __init__(self):
        self.rows = {}

    def __getattr__(self, name):
        unit = {"vlr_gemv_workspace_bytes": 1, "vlr_gemv_w4_workspace_bytes": 2, "vlr_gemv_lora_workspace_bytes": 3, "vlr_gemv_lora_u_bytes": 5,
                "vlr_gemv_wide_workspace_bytes": 7, "vlr_gemv_wide_lora_workspace_bytes": 11, "vlr_gemv_wide_lora_u_bytes": 13,
                "vlr_attn_decode_workspace_bytes": 0}.get(name)
        if unit is None:
            raise AttributeError(name)

        def fn(M, *rest):
            self.rows.setdefault(name, set()).add(M)
            return 64 if name == "vlr_attn_decode_workspace_bytes" else 16 * unit * M
        return fn


def decode_ws(monkeypatch, B, lora=None, packed=None, wide_gemv=True):
    import vlrlhf.engine as E
    lib = StubLib()
    monkeypatch.setattr(E._hip, "lib", lambda: lib)
    eng = SimpleNamespace(_ws={}, lora=lora, lora_layout=SimpleNamespace(qkv_targets=3), packed=packed, wide_gemv=wide_gemv, Nqkv=48, H=16, Nq=16,
                          I=32, V=40, nh=1, dev=torch.device("cpu"), RDT=torch.bfloat16)
    d = E.LlavaHipEngine._decode_ws(eng, B, 50)
    assert E.LlavaHipEngine._decode_ws(eng, B, 50) is d, "cached per shape"
    assert d["struct"].gemv_ws_bytes == d["gemv"].numel()
    return d, lib.rows


def test_decode_ws_is_sized_for_64_row_groups_when_the_wide_path_can_run(monkeypatch):
    # up to 16 rows: nothing changes, the wide helpers are never asked
    d, rows = decode_ws(monkeypatch, 16)
    assert d["gemv"].numel() == 16 * 16 and not any("wide" in k for k in rows) and "u" not in d
    # 20 rows: min(B, 64) rows of wide scratch; the 16-row helpers are still asked for 16
    d, rows = decode_ws(monkeypatch, 20)
    assert d["gemv"].numel() == 16 * 7 * 20 and rows["vlr_gemv_wide_workspace_bytes"] == {20} and rows["vlr_gemv_workspace_bytes"] == {16}
    d, rows = decode_ws(monkeypatch, 100)
    assert d["gemv"].numel() == 16 * 7 * 64 and rows["vlr_gemv_wide_workspace_bytes"] == {64}
    # live adapters: the adapter slice and the u scratch too
    d, rows = decode_ws(monkeypatch, 33, lora={"r": 8})
    assert d["gemv"].numel() == 16 * 11 * 33 and d["u"].numel() == 16 * 13 * 33 == d["lora_struct"].u_bytes
    assert rows["vlr_gemv_wide_lora_workspace_bytes"] == rows["vlr_gemv_wide_lora_u_bytes"] == {33}
    d, rows = decode_ws(monkeypatch, 12, lora={"r": 8})
    assert d["gemv"].numel() == 16 * 3 * 12 and d["u"].numel() == 16 * 5 * 12 and not any("wide" in k for k in rows)
    # packed weights keep 16-row groups; so does an engine told to
    d, rows = decode_ws(monkeypatch, 33, packed={})
    assert d["gemv"].numel() == 16 * 2 * 16 and not any("wide" in k for k in rows)
    d, rows = decode_ws(monkeypatch, 33, wide_gemv=False)
    assert d["gemv"].numel() == 16 * 16 and not any("wide" in k for k in rows)


def test_lm_head_rows_take_the_wide_call_only_with_wide_scratch(monkeypatch):
    import vlrlhf.engine as E
    calls = []
    monkeypatch.setattr(E._hip, "call", lambda name, *a: calls.append((name, a[15], a[1].shape[0])))
    monkeypatch.setattr(E._hip, "lib", lambda: SimpleNamespace(vlr_gemv_wide_workspace_bytes=lambda M, N, K: 100 * M))
    eng = SimpleNamespace(hd=128, max_pos=64, wide_gemv=True)
    X, Y, W = torch.zeros(70, 8), torch.zeros(70, 4), torch.zeros(4, 8)
    run = lambda M, nbytes: (calls.clear(), E.LlavaHipEngine._gemv_rows(eng, 1, X[:M], W, Y[:M], M, 4, 8, torch.empty(nbytes, dtype=torch.uint8)),  # noqa: E731
                             list(calls))[2]
    assert run(70, 6400) == [("vlr_gemv_wide_bf16", 64, 64), ("vlr_gemv_wide_bf16", 6, 6)]
    assert run(33, 3300) == [("vlr_gemv_wide_bf16", 33, 33)]
    assert run(33, 3299) == [("vlr_gemv_bf16", 16, 16), ("vlr_gemv_bf16", 16, 16), ("vlr_gemv_bf16", 1, 1)], "scratch sized for 16 rows: groups"
    assert run(16, 6400) == [("vlr_gemv_bf16", 16, 16)]
    eng.wide_gemv = False
    assert run(33, 6400) == [("vlr_gemv_bf16", 16, 16), ("vlr_gemv_bf16", 16, 16), ("vlr_gemv_bf16", 1, 1)]


# ---- VLPPOTrainer.generate(batch_size=k): trl's _generate_batched
EOS, PAD = 2, 0


class ScriptedPolicy:
    """generate() answers each row with (last prompt token + 100, + 101, EOS, PAD) and records what it was given"""

    config = {}

    def __init__(self):
        self.calls = []

    def generate(self, input_ids=None, attention_mask=None, **kw):
        self.calls.append(dict(ids=input_ids.clone(), mask=attention_mask.clone(), kw=kw))
        last = input_ids[:, -1:]
        return torch.cat([input_ids, last + 100, last + 101, torch.full_like(last, EOS), torch.full_like(last, PAD)], 1)


def ppo_generate(queries, **kw):
    from vlrlhf.base.trainer import VLPPOTrainer
    model = ScriptedPolicy()
    me = SimpleNamespace(generation_kwargs=dict(eos_token_id=EOS, do_sample=False), is_peft_model=False, padding_value=PAD, model=model,
                         accelerator=SimpleNamespace(device=torch.device("cpu")))
    me._generate_rows = lambda *a: VLPPOTrainer._generate_rows(me, *a)
    return VLPPOTrainer.generate(me, queries, **kw), model.calls


def test_ppo_generate_in_chunks_keeps_order_and_pads_each_chunk():
    t = lambda *x: torch.tensor(x, dtype=torch.long)      # noqa: E731
    queries = [t(5), t(6, 7, 8), t(9, 10), t(11, 12, 13, 14), t(15)]
    px, names = torch.arange(5.0)[:, None], list("abcde")
    want = [t(int(q[-1]) + 100, int(q[-1]) + 101, EOS) for q in queries]
    whole, calls = ppo_generate(queries, pixel_values=px, img_path=names, flag=7)
    assert len(calls) == 1 and calls[0]["ids"].shape == (5, 4), "batch_size=None: one call, padded to the longest query"
    assert all(torch.equal(a, b) for a, b in zip(whole, want))
    out, calls = ppo_generate(queries, batch_size=2, pixel_values=px, img_path=names, flag=7)
    assert all(torch.equal(a, b) for a, b in zip(out, want)), "the responses come back in the queries' order"
    assert [c["ids"].shape for c in calls] == [(2, 3), (2, 4), (1, 1)], "chunks of 2, 2, 1 rows, each padded to ITS longest query"
    assert calls[0]["ids"].tolist() == [[PAD, PAD, 5], [6, 7, 8]] and calls[0]["mask"].tolist() == [[0, 0, 1], [1, 1, 1]], "left padding"
    assert calls[1]["ids"].tolist() == [[PAD, PAD, 9, 10], [11, 12, 13, 14]] and calls[2]["ids"].tolist() == [[15]]
    assert [c["kw"]["pixel_values"].flatten().tolist() for c in calls] == [[0.0, 1.0], [2.0, 3.0], [4.0]], "per-query image inputs follow their rows"
    assert [c["kw"]["img_path"] for c in calls] == [["a", "b"], ["c", "d"], ["e"]] and all(c["kw"]["flag"] == 7 for c in calls)
    for k in (5, 32):
        out, calls = ppo_generate(queries, batch_size=k, pixel_values=px)
        assert len(calls) == 1 and calls[0]["ids"].shape == (5, 4), "a batch that fits one chunk is today's single call"
        assert all(torch.equal(a, b) for a, b in zip(out, want))
    both, _ = ppo_generate(queries, batch_size=3, return_prompt=True)
    assert all(torch.equal(b, torch.cat([q, w])) for b, q, w in zip(both, queries, want))
    with pytest.raises(ValueError, match="batch_size"):
        ppo_generate(queries, batch_size=0)


def test_ppo_train_samples_32_rows_at_a_time():
    import inspect
    from vlrlhf.base.trainer import VLPPOTrainer
    assert inspect.signature(VLPPOTrainer.generate).parameters["batch_size"].default is None
    assert "batch_size=32" in inspect.getsource(VLPPOTrainer.train)
