"""bench.py's command line on CPU: the self-spawn of `--gpus N` and the CPU-worker mode (no HIP device needed)."""
import importlib.util
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gpus_n_respawns_itself_under_torch_distributed_run(monkeypatch):
    """`python bench.py --gpus 4` outside torchrun must start 4 ranks (round 1's --gpus was parsed and ignored)."""
    import argparse
    import torch
    bench = _bench()
    calls = []
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 8)
    monkeypatch.setattr(bench.subprocess, "call", lambda cmd, env=None: calls.append((cmd, env)) or 0)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7"])
    with pytest.raises(SystemExit) as exc:
        bench.spawn_ranks_if_needed(argparse.Namespace(gpus=4))
    assert exc.value.code == 0 and len(calls) == 1
    cmd, env = calls[0]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == ["--gpus", "4", "--steps", "7"] and cmd[-5].endswith("bench.py")
    assert env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_gpus_n_is_a_no_op_under_torchrun_and_at_one_gpu(monkeypatch):
    import argparse
    bench = _bench()
    monkeypatch.setattr(bench.subprocess, "call", lambda *a, **k: (_ for _ in ()).throw(AssertionError("must not spawn")))
    monkeypatch.setenv("WORLD_SIZE", "4")
    bench.spawn_ranks_if_needed(argparse.Namespace(gpus=4))      # already a rank
    monkeypatch.delenv("WORLD_SIZE")
    bench.spawn_ranks_if_needed(argparse.Namespace(gpus=1))      # single GPU


def test_gpus_n_refuses_when_devices_are_missing(monkeypatch):
    import argparse
    import torch
    bench = _bench()
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    with pytest.raises(SystemExit, match="only 1 HIP device"):
        bench.spawn_ranks_if_needed(argparse.Namespace(gpus=8))


def test_cpu_worker_mode_times_one_frame():
    """The 'all cores' CPU figure starts one `bench.py --cpu-worker` per core; the worker must not need torch or a GPU."""
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu-worker", "300", "5"], cwd=ROOT)
    assert float(out.decode().strip()) > 0


def test_dump_outputs_writes_float32_files_and_a_seeded_row_sample(tmp_path, monkeypatch):
    """--dump-outputs: every array as <name>.npy in float32, whole while it fits the budget; above it, the same sorted rows of
    every array, the same rows from run to run."""
    import numpy as np
    import torch
    bench = _bench()
    g = torch.Generator().manual_seed(0)
    arrays = {"radial": torch.randn(500, 112, generator=g), "angular": torch.randn(500, 896, generator=g),
              "position_grad": torch.randn(500, 3, generator=g)}
    bench.dump_outputs(str(tmp_path / "whole"), arrays)
    for k, v in arrays.items():
        a = np.load(tmp_path / "whole" / f"{k}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, v.numpy())
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 100 * (112 + 896 + 3) * 4)       # room for 100 of the 500 rows
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays)
    total = sum(os.path.getsize(tmp_path / "a" / f"{k}.npy") for k in arrays)
    assert total <= bench.DUMP_LIMIT_BYTES + 3 * 128                                 # (+ one .npy header per file)
    rows = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in arrays}
    assert all(a.shape[0] == 100 for a in rows.values())
    keep = [int(np.flatnonzero((arrays["position_grad"].numpy() == r).all(1))[0]) for r in rows["position_grad"]]
    assert keep == sorted(keep) and len(set(keep)) == 100
    for k, v in arrays.items():
        assert np.array_equal(rows[k], v.numpy()[keep])
        assert np.array_equal(np.load(tmp_path / "b" / f"{k}.npy"), rows[k])


def test_plain_run_leaves_the_extra_runs_to_full():
    """Without --full a run has no CPU baseline, no rocprofv3 pass and no side line; --full brings them all back, and the --no-*
    switches still take single ones out of a full run."""
    bench = _bench()
    plain = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not plain.full and plain.no_cpu_baseline and plain.no_side and plain.no_pmc
    assert (plain.steps, plain.warmup, plain.settle, plain.workload) == (20, 5, -1, "aev")
    full = bench.parse_args(["--steps", "20", "--warmup", "5", "--full"])
    assert full.full and not (full.no_cpu_baseline or full.no_side or full.no_pmc)
    part = bench.parse_args(["--full", "--no-side", "--no-pmc"])
    assert part.no_side and part.no_pmc and not part.no_cpu_baseline
    assert bench.parse_args(["--workload", "cfconv"]).no_cpu_baseline


@pytest.mark.parametrize("full", [False, True])
def test_side_lines_run_with_full_only(monkeypatch, capsys, full):
    """main() at N = 1: a plain run prints the headline alone (with an empty side_errors); --full runs and attaches every side line."""
    import json
    bench = _bench()
    ran = []

    class OneRank:
        rank, world = 0, 1

        def close(self):
            pass
    monkeypatch.setattr(bench, "Ranks", OneRank)
    monkeypatch.setattr(bench, "run_aev", lambda args, R: ran.append(("aev", args.no_cpu_baseline, args.no_pmc)) or {"value": 1.0})
    for name in ("latency", "torchani", "cfconv", "cfconv_reference", "conformers", "neighbors"):
        monkeypatch.setitem(bench.WORKLOADS, name, lambda args, R, name=name: ran.append(name) or {"value": 2.0})
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"] + (["--full"] if full else []))
    bench.main()
    line = json.loads(capsys.readouterr().out.strip())
    assert line["side_errors"] == {}
    if full:
        assert ran == [("aev", False, False), "latency", "torchani", "cfconv", "cfconv_reference", "conformers", "neighbors"]
        assert set(line["side"]) == set(ran[1:])
    else:
        assert ran == [("aev", True, True)] and "side" not in line


@pytest.mark.parametrize("argv, message", [(["--steps", "0"], "--steps must be at least 1"),
                                           (["--dump-outputs", "d", "--workload", "cfconv"], "--dump-outputs writes")])
def test_command_line_refuses_what_it_cannot_time_or_dump(argv, message):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 2 and message in out.stderr, out.stderr
