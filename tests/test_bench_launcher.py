"""CPU test of bench.py's own launcher: `python bench.py --gpus N` (no WORLD_SIZE in the environment) must start N rank
processes itself, rendezvous them over 127.0.0.1, print ONE JSON line from rank 0 whose n_gpus is the number of ranks the
process group saw, and hand a failing rank's exit code back.  --dry-run keeps it on the CPU (gloo, no HIP library)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--steps", "3", "--warmup", "1", *extra],
                          env=env, capture_output=True, text=True, timeout=240)


@pytest.mark.timeout(300)
def test_gpus_2_launches_two_ranks_unwrapped():
    r = _run("--gpus", "2", "--full")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout                      # one line, from rank 0 only
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 3 and line["warmup"] == 1
    for key in ("metric", "value", "unit", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                "roofline", "cpu_baseline"):
        assert key in line, key
    # the N > 1 line's diagnostics under --full (bench.comm_diagnostics, the same code the RCCL run goes through): payload, a
    # stand-alone all-reduce's algorithm / bus bandwidth, the step with its collectives stubbed, every rank's launch mode
    assert line["ranks_seen"] == 2
    assert line["allreduce_payload_mb"] == round(4 * (3 * 4096 + 2048 + 512) / 1e6, 2) and len(line["allreduce_messages_mb"]) == 5
    assert line["allreduce_standalone_ms"] > 0 and line["allreduce_bus_gbs"] == pytest.approx(line["allreduce_alg_gbs"], abs=0.11)   # 2 (N - 1) / N = 1
    assert line["launch_mode_per_rank"] == ["dry run (rank 0)", "dry run (rank 1)"]
    assert line["ms_per_step_collectives_stubbed"] > 0
    assert line["comm_exposed_ms"] == pytest.approx(line["ms_per_step"] - line["ms_per_step_collectives_stubbed"], abs=2e-3)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("n", [4, 8])
def test_gpus_4_and_8_report_the_ranks_seen(n):
    """The driver's scaling run is `--gpus 1, 2, 4, 8` back to back: both launch forms at 4 and 8 ranks -- bench.py's own
    launcher, and `python -m torch.distributed.run --nproc-per-node N` with bench.py as one of the ranks (the driver's form)."""
    r = _run("--gpus", str(n))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == n, r.stdout
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
                        "--master-port", str(29600 + n), os.path.join(ROOT, "bench.py"), "--dry-run", "--gpus", str(n), "--steps", "3",
                        "--warmup", "1"], env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == n, r.stdout


@pytest.mark.timeout(300)
def test_a_failing_rank_fails_the_launch():
    r = _run("--gpus", "2", "--dry-run-fail-rank", "1")
    assert r.returncode == 3, (r.returncode, r.stderr[-2000:])
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_world_size_must_match_gpus():
    r = _run("--gpus", "2", env_extra={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr


def test_single_rank_needs_no_launcher():
    r = _run("--gpus", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])["n_gpus"] == 1


def test_plain_run_times_the_headline_only():
    """A plain run drops every leg beside the timed steps; --full brings them back, and a --no-* switch still drops one."""
    import bench
    legs = ("no_cpu_baseline", "no_roofline", "no_generator", "no_inference", "no_wino_split", "no_engine_api", "no_live_pmc")
    plain, full, full_but = bench.parse([]), bench.parse(["--full"]), bench.parse(["--full", "--no-roofline"])
    assert not plain.full and all(getattr(plain, k) for k in legs) and plain.dump_outputs is None
    assert full.full and not any(getattr(full, k) for k in legs)
    assert full_but.no_roofline and not any(getattr(full_but, k) for k in legs if k != "no_roofline")
    assert bench.parse(["--steps", "7", "--dump-outputs", "d"]).steps == 7
    r = _run("--gpus", "2")                               # the N > 1 diagnostics are a --full leg
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 3 and line["ms_per_step"] > 0
    assert "comm_exposed_ms" not in line and "allreduce_payload_mb" not in line


def test_dump_outputs_of_the_full_step(tmp_path):
    """--dump-outputs on a stand-in of the full-step workload (CPU tensors): the logged scalars as float64, the generator state
    whole, the discriminator state as a seeded sample that is the same from call to call; every file float32 / float64."""
    import numpy as np
    import torch
    import bench

    class _Logged:
        pending = (["a", "b", "c"], torch.tensor([1.5, -2.0, 3.25]), None, 1e-4)

    class _Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            torch.manual_seed(0)
            self.Generator = torch.nn.Linear(8, 4)
            self.Discriminator = torch.nn.Linear(300, 200)       # 60 000 weights > DUMP_SAMPLE: sampled

    class _Wl:
        name, graphed, model, _logged = "full_step", None, _Model(), _Logged()

    wl = _Wl()
    bench.dump_outputs(wl, str(tmp_path / "one"))
    bench.dump_outputs(wl, str(tmp_path / "two"))
    got = {p.stem: np.load(p) for p in sorted((tmp_path / "one").glob("*.npy"))}
    assert set(got) == {"logged_scalars", "generator_state", "discriminator_state_sample"}
    assert got["logged_scalars"].dtype == np.float64 and got["logged_scalars"].tolist() == [1.5, -2.0, 3.25]
    g = wl.model.Generator
    assert np.array_equal(got["generator_state"], torch.cat([g.weight.reshape(-1), g.bias]).detach().numpy())
    d = got["discriminator_state_sample"]
    assert d.dtype == np.float32 and d.size == bench.DUMP_SAMPLE + 200
    assert np.isin(d[:bench.DUMP_SAMPLE], wl.model.Discriminator.weight.detach().numpy().reshape(-1)).all()
    for k, v in got.items():
        assert np.array_equal(v, np.load(tmp_path / "two" / (k + ".npy"))), k
