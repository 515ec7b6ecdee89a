"""`python bench.py --gpus N` without torchrun launches its own N ranks (one fresh child
process per GPU with the torchrun environment) and relays rank 0's JSON line.  CPU: the
dry-run hook stops every child before any device work and prints its environment; a
child that fails makes the launcher fail.  GPU: two ranks of the real bench on the box's
one GPU (gloo rehearsal: RCCL refuses two ranks on one device) report n_gpus 2."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(kw)
    return env


def test_launcher_spawns_n_ranks_with_torchrun_env():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "3", "--launch-dry-run"], capture_output=True, text=True,
                       env=_env(BGCN_DIST_BACKEND="gloo"), timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.strip().splitlines()]
    assert [d["RANK"] for d in lines] == ["0", "1", "2"]
    assert [d["LOCAL_RANK"] for d in lines] == ["0", "1", "2"]
    assert {d["WORLD_SIZE"] for d in lines} == {"3"}
    assert {d["MASTER_ADDR"] for d in lines} == {"127.0.0.1"}
    assert len({d["MASTER_PORT"] for d in lines}) == 1 and int(lines[0]["MASTER_PORT"]) > 0
    assert {d["BGCN_DIST_BACKEND"] for d in lines} == {"gloo"}


def test_launcher_under_torchrun_env_does_not_respawn():
    # WORLD_SIZE present (torchrun launched us): the process is one rank, not a launcher
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--launch-dry-run"], capture_output=True, text=True,
                       env=_env(WORLD_SIZE="2", RANK="1", LOCAL_RANK="1"), timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and json.loads(lines[0])["RANK"] == "1"


def test_launcher_fails_when_a_rank_fails():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--workload", "no_such_workload"],
                       capture_output=True, text=True, env=_env(), timeout=120)
    assert r.returncode != 0
    assert "exited with status" in r.stderr


def test_full_and_dump_outputs_are_options(tmp_path):
    # the dry run stops before any device work: both options parse, nothing is written
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--full",
                        "--dump-outputs", str(out), "--launch-dry-run"], capture_output=True, text=True,
                       env=_env(), timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(r.stdout.strip().splitlines()) == 1
    assert not out.exists()


# the keys of the result line that only a --full run measures
FULL_LEGS = ("dense_path", "dropin_path", "eval_path", "aggregation_5000", "compaction_standalone", "staging",
             "dropedge_host_once_untimed")


def _bench_line(*argv):
    r = subprocess.run([sys.executable, "-u", BENCH, "--gpus", "1", *argv], capture_output=True, text=True,
                       env=_env(), timeout=110, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain_runs(tmp_path_factory):
    """Two plain runs with the same arguments, each with its own dump: [(line, {file: array})]."""
    import numpy as np
    runs = []
    for k in range(2):
        out = tmp_path_factory.mktemp(f"dump{k}")
        line = _bench_line("--steps", "3", "--warmup", "2", "--pool", "2", "--dump-outputs", str(out))
        runs.append((line, {f.name: np.load(f) for f in out.iterdir()}))
    return runs


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_outputs(plain_runs):
    """A plain run prints the headline line without the --full legs and --dump-outputs writes
    the last timed step's loss, gradients, parameters and activations as float32 .npy."""
    import numpy as np
    line, files = plain_runs[0]
    assert line["steps"] == 3 and line["warmup"] == 2
    assert line["unit"] == "trees/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / 128 - 1.0) < 1e-3    # value = trees / step time
    assert line["invalid_steps"] == 0 and line["status"] == 0
    assert line["cpu_baseline"] is None
    for leg in FULL_LEGS:
        assert leg not in line
    assert {"loss.npy", "H1.npy", "H2.npy", "param.fc.weight.npy", "grad.fc.weight.npy",
            "param.TDrumorGCN.conv1.lin.weight.npy", "grad.BUrumorGCN.conv2.lin.weight.npy"} <= set(files)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 * 2**20
    assert abs(float(files["loss.npy"][0]) - line["final_loss"]) <= 1e-5
    assert files["H1.npy"].shape[1] == 128 and files["H1.npy"].shape == files["H2.npy"].shape
    assert files["grad.fc.weight.npy"].shape == files["param.fc.weight.npy"].shape == (4, 256)
    assert np.abs(files["grad.TDrumorGCN.conv1.lin.weight.npy"]).max() > 0


@pytest.mark.gpu
def test_same_arguments_dump_identical_outputs(plain_runs):
    """Pool, initial parameters, dropout and DropEdge seeds are fixed and the step is
    deterministic: two runs with the same arguments write the same arrays, bit for bit."""
    import numpy as np
    (_, a), (_, b) = plain_runs
    assert set(a) == set(b)
    for name in sorted(a):
        assert np.array_equal(a[name], b[name]), name


@pytest.mark.gpu
def test_full_run_reports_every_leg():
    """--full brings back every leg a plain run leaves out (each at its smallest size), beside
    the same headline fields."""
    line = _bench_line("--full", "--steps", "3", "--warmup", "2", "--pool", "2", "--cpu-trees", "4",
                       "--cpu-steps", "1", "--cpu-warmup", "1", "--cpu-repeats", "1", "--host-fed-trees", "512",
                       "--host-fed-workers", "2")
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["invalid_steps"] == 0 and line["status"] == 0
    for leg in FULL_LEGS:
        assert leg in line, leg
    assert line["cpu_baseline"]["value"] > 0
    assert line["dense_path"]["value"] > 0 and line["eval_path"]["value"] > 0
    assert line["dropin_path"]["value"] > 0 and line["dropin_path"]["prepared_ahead"]["value"] > 0
    assert line["staging"]["host_fed"]["value"] > 0 and line["staging"]["host_fed_dataloader"]["value"] > 0
    assert line["compaction_standalone"]["paced"]["frac"] > 0 and line["aggregation_5000"]["td"]["frac"] > 0


@pytest.mark.gpu
def test_bench_two_ranks_on_one_gpu():
    r = subprocess.run([sys.executable, "-u", BENCH, "--gpus", "2", "--steps", "2", "--warmup", "1", "--pool", "2",
                        "--no-cpu-baseline"], capture_output=True, text=True,
                       env=_env(BGCN_DIST_BACKEND="gloo"), timeout=110, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2
    assert line["config"]["parallelism"] == "dp2"
    assert line["invalid_steps"] == 0 and line["status"] == 0
    assert line["value"] > 0
