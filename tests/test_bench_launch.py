"""`python bench.py --gpus N` without a launcher must start N ranks itself (one per GPU, torch.distributed.run on 127.0.0.1)
and print ONE JSON line with n_gpus = N.  CPU check of that path with 2 gloo ranks and no model (--dry_run_launch); the
real thing runs on RCCL when the driver launches the scaling bench."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=300, env=e)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_self_launches_two_ranks():
    line = _run(["--gpus", "2", "--steps", "3", "--warmup", "1", "--dry_run_launch"])
    assert line["n_gpus"] == 2 and line["rccl_ranks"] == 2 and line["steps"] == 3
    assert abs(line["mean_rank"] - 0.5) < 1e-9          # the metric all-reduce saw both ranks


def test_bench_self_launches_eight_ranks():
    """the driver's largest scaling point, as far as a CPU can take it: 8 gloo ranks through the same self-launch, barrier / max-over-ranks
    timing, metric all-reduce and bucket probe (bound 0 and 16: two records), ONE JSON line"""
    line = _run(["--gpus", "8", "--steps", "2", "--warmup", "1", "--dry_run_launch"], env={"OMP_NUM_THREADS": "1"})
    assert line["n_gpus"] == 8 and line["rccl_ranks"] == 8
    assert abs(line["mean_rank"] - 3.5) < 1e-9
    probe = line["comm"]["bucket_probe"]
    assert [p["channel_bound"] for p in probe] == [0, 16] and all("error" not in p and p["busbw_gbps"] > 0 for p in probe), probe


def test_rccl_init_log_parsing(tmp_path):
    """bench.rccl_debug_channels reads the channel counts RCCL says it created, per communicator, from its INIT log"""
    sys.path[:0] = [ROOT]
    import importlib
    bench = importlib.import_module("bench")
    log = tmp_path / "rccl.log"
    log.write_text("h:1:1 [0] NCCL INFO comm 0x1 rank 0 nRanks 8 nNodes 1 localRanks 8 localRank 0 MNNVL 0\n"
                   "h:1:1 [0] NCCL INFO 32 coll channels, 0 collnet channels, 0 nvls channels, 32 p2p channels, 4 p2p channels per peer\n"
                   "h:1:1 [0] NCCL INFO 16 coll channels, 0 collnet channels, 0 nvls channels, 16 p2p channels, 2 p2p channels per peer\n")
    assert bench.rccl_debug_channels(str(log)) == [32, 16]
    log.write_text("NCCL INFO Channel 00/24 : 0 1 2 3\nNCCL INFO Channel 01/24 : 0 1 2 3\nNCCL INFO Channel 00/16 : 0 1\n")
    assert bench.rccl_debug_channels(str(log)) == [24, 16]
    assert bench.rccl_debug_channels(str(tmp_path / "missing")) == [] and bench.rccl_debug_channels(None) == []


def test_bench_single_rank_needs_no_launcher():
    line = _run(["--gpus", "1", "--steps", "2", "--warmup", "0", "--dry_run_launch"])
    assert line["n_gpus"] == 1


def test_relaunch_passes_arguments_and_exit_code(tmp_path):
    sys.path[:0] = [os.path.join(ROOT, "vl-rlhf_amd")]
    from vlrlhf.parallel import relaunch_under_torchrun
    script = tmp_path / "w.py"
    script.write_text("import os, sys\nassert os.environ['WORLD_SIZE'] == '2' and os.environ['MASTER_ADDR'] == '127.0.0.1'\n"
                      "assert sys.argv[1:] == ['--x', '7']\nsys.exit(0 if os.environ['LOCAL_RANK'] in '01' else 3)\n")
    assert relaunch_under_torchrun(str(script), ["--x", "7"], 2) == 0


def test_dump_outputs_cpu(tmp_path):
    """bench.dump_outputs (--dump-outputs DIR): float32 / float64 .npy files only, a fixed seeded sample of the flat buffers (the same
    positions every run), within 64 MB, and the last step's loss and metrics"""
    sys.path[:0] = [ROOT]
    import importlib
    import numpy as np
    import torch
    from collections import defaultdict
    from types import SimpleNamespace
    bench = importlib.import_module("bench")
    n = (1 << 20) + 12345
    g = torch.Generator().manual_seed(0)
    eng = SimpleNamespace(lora=None, policy=SimpleNamespace(flat=torch.randn(n, generator=g).bfloat16()), master=torch.randn(n, generator=g),
                          m=torch.randn(n, generator=g), v=torch.rand(n, generator=g), grads=torch.randn(n, generator=g).bfloat16(),
                          norm_out=torch.tensor([3.0, 0.25, 9.0]))
    tr = SimpleNamespace(_stored_metrics=defaultdict(lambda: defaultdict(list)))
    for step in range(3):
        tr._stored_metrics["train"]["rewards/chosen"].append(torch.tensor(float(step)))
        tr._stored_metrics["train"]["logps/rejected"].append(torch.tensor(-10.0 - step))
    outs = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch.tensor(0.6931), tr, eng)
        outs.append({f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = outs
    assert set(a) == {"loss", "grad_norm", "metric_rewards_chosen", "metric_logps_rejected", "weights", "master", "adam_m", "adam_v", "grads",
                      "sample_index"}
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert all(np.array_equal(a[k], b[k]) for k in a)
    idx = a["sample_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE and idx.min() >= 0 and idx.max() < n
    assert np.array_equal(a["master"], eng.master.numpy()[idx]) and np.array_equal(a["weights"], eng.policy.flat.float().numpy()[idx])
    assert a["metric_rewards_chosen"][0] == 2.0 and a["metric_logps_rejected"][0] == -12.0 and abs(a["loss"][0] - 0.6931) < 1e-6
