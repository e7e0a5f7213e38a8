"""bench.py's own rank launcher (CPU): `python bench.py --gpus N` with no WORLD_SIZE starts N
ranks through torch.distributed.run (light_training/launch.py:81-112 re-launches the same way);
as a rank, or with N = 1, it does not relaunch.  Also its host-side options: a plain run
switches the roofline / parity / CPU-baseline legs off (--full brings them back), and
--dump-outputs writes float32 arrays within its byte budget, sampled at fixed indices."""
import os
import sys
from types import SimpleNamespace

import bench


def test_launcher_cmd_shape():
    cmd = bench.launcher_cmd(["--gpus", "4", "--steps", "7"], 4, 29555)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    i = cmd.index("--master-addr")
    assert cmd[i + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29555"
    j = cmd.index(os.path.abspath(bench.__file__))
    assert cmd[j + 1:] == ["--gpus", "4", "--steps", "7"]


def test_no_relaunch_as_rank_or_single_gpu(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert bench.maybe_launch_ranks(SimpleNamespace(gpus=2)) is None
    monkeypatch.delenv("WORLD_SIZE")
    assert bench.maybe_launch_ranks(SimpleNamespace(gpus=1)) is None


def test_relaunch_runs_child(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    seen = {}

    def fake_call(cmd):
        seen["cmd"] = cmd
        return 3
    import subprocess
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8"])
    assert bench.maybe_launch_ranks(SimpleNamespace(gpus=8)) == 3
    assert "--nproc-per-node=8" in seen["cmd"] and seen["cmd"][-2:] == ["--gpus", "8"]


def test_plain_run_switches_the_extra_legs_off(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert (a.op_timers, a.parity, a.cpu_baseline) == (0, 0, 0)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--parity", "0"])
    a = bench.parse()
    assert a.full and (a.op_timers, a.parity, a.cpu_baseline) == (1, 0, 1)


def test_dump_outputs_names_budget_and_fixed_sample(tmp_path, monkeypatch):
    import numpy as np
    import torch
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 4 * 100)  # 4 arrays x 100 floats
    big = torch.arange(1000, dtype=torch.float64).reshape(10, 100).t()  # non-contiguous view
    outs = [torch.ones(2, 3), big]
    hfs = [[{"aad": torch.zeros(5), "ada": torch.full((7,), 2.0).half()}], []]
    for d in ("a", "b"):
        shapes = bench.dump_outputs(str(tmp_path / d), (outs, hfs))
    assert shapes == {"out0": [2, 3], "out1": [100], "hf0_0_aad": [5], "hf0_0_ada": [7]}
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in shapes}
    assert all(v.dtype == np.float32 for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 4 * 4 * 100
    assert np.array_equal(got["out0"], np.ones((2, 3))) and np.array_equal(got["hf0_0_ada"],
                                                                          np.full(7, 2.0))
    # the sample: elements of the logical (row-major) order, the same ones in every run
    flat = big.reshape(-1).numpy()
    assert np.isin(got["out1"], flat).all() and len(np.unique(got["out1"])) > 50
    assert np.array_equal(got["out1"], np.load(tmp_path / "b" / "out1.npy"))
    # a bare tensor (the full model's logits) is one array named "out"
    assert bench.dump_outputs(str(tmp_path / "c"), torch.ones(3)) == {"out": [3]}


def test_stamp_marks_rehearsal(monkeypatch):
    monkeypatch.setenv("WF_BENCH_BACKEND", "gloo")
    out = bench._stamp({}, SimpleNamespace(devices=1), 2)
    assert out["devices"] == 1 and "2 ranks on 1 GPU" in out["rehearsal"]
    assert "rehearsal" not in bench._stamp({}, SimpleNamespace(devices=8), 8)
