"""bench.py's multi-GPU path without devices: `--gpus N --dry-run` builds the N
ranks' launch environments, checks both scaling modes' window partitions and assembles + validates the
record an N-rank run prints (synthetic timings, marked as such).  No GPU, no RCCL."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(*extra):
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--dry-run"] + list(extra),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, "ONE JSON line expected, got %d" % len(lines)
    return json.loads(lines[0])


@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_dry_run_record_schema(n):
    r = run("--gpus", str(n), "--steps", "5", "--warmup", "1", "--full")
    assert r["n_gpus"] == n and r["ranks"] == n and r["steps"] == 5 and r["warmup"] == 1
    assert r["data"].startswith("DRY RUN")
    assert r["scaling"] == "weak" and r["config"]["sequences"] == n
    assert r["vs_baseline"] is None and r["higher_is_better"] is True and r["dtype"] == "f64"
    rf = r["roofline"]
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic", "frac_events", "whole_step_frac",
                "traffic_ratio")) <= set(rf)
    assert 0.0 < rf["whole_step_frac"] < 1.0
    if n > 1:
        assert len(r["per_rank_ms_per_step"]) == n and r["ranks_source"] == "ncclCommCount"
        assert r["allreduce"]["bytes"] == (64 * 64 + 64 * 32 + 64 + 64 * 32 * 32 + 1) * 8
        for leg in ("epoch", "minibatch_s64"):
            assert r["strong_scaling"][leg]["scaling"] == "strong"
    else:
        assert "per_rank_ms_per_step" not in r and r["ranks_source"] == "no communicator"
    # the headline region spans >= 5 s of GPU time by default (a coarse utilisation sampler sees it)
    assert r["reps"] * r["steps"] * 3.1e-3 >= 4.8


@pytest.mark.parametrize("n", [1, 2])
def test_plain_dry_run_times_one_block(n):
    """Without --full the run times exactly --steps steps (one block) and carries no strong-scaling
    side record; only the dominant kernel (and the all-reduce) is bracketed."""
    r = run("--gpus", str(n), "--steps", "7", "--warmup", "2")
    assert r["steps"] == 7 and r["warmup"] == 2 and r["reps"] == 1 and len(r["ms_per_step_reps"]) == 1
    assert r["ms_per_step"] > 0 and "strong_scaling" not in r
    assert set(r["kernels"]) <= {"stats", "allreduce"}


@pytest.mark.gpu
def test_plain_run_times_steps_and_dumps_outputs(tmp_path):
    """A plain run on the device: one block of exactly --steps timed steps, none of --full's records, and
    --dump-outputs writes the packed statistics of the last timed step (float64, as the caller gets them)."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["steps"] == 3 and r["reps"] == 1 and len(r["ms_per_step_reps"]) == 1
    assert r["ms_per_step"] > 0 and r["value"] > 1e9 and r["dtype"] == "f64"
    assert not set(r) & {"minibatch_s64", "f32_mode", "whole_chain", "cpu_baseline", "c2_k16_d8", "c5_k256_d64",
                         "strong_scaling"}
    K, D, rows = 64, 32, (1000000 // 257) * 257
    shapes = {"A_raw": (K, K), "xbar": (K, D), "neff": (K,), "S": (K, D, D), "lb": (1,)}
    out = {}
    for name, shape in shapes.items():
        out[name] = np.load(str(tmp_path / (name + ".npy")))
        assert out[name].shape == shape and out[name].dtype == np.float64 and np.all(np.isfinite(out[name]))
    # posteriors sum to one: the wrap transition statistic and the state counts each sum to the row count
    assert abs(out["A_raw"].sum() / rows - 1.0) < 1e-9 and abs(out["neff"].sum() / rows - 1.0) < 1e-9


def test_dry_run_strong_scaling_line():
    r = run("--gpus", "8", "--scaling", "strong")
    assert r["scaling"] == "strong" and r["config"]["sequences"] == 1
    assert "windows[rank::N]" in r["config"]["parallelism"]


def test_rank_environments():
    sys.path.insert(0, REPO)
    import bench
    envs = bench.rank_envs(8, 29511, base={"PATH": "/usr/bin"})
    assert [e["RANK"] for e in envs] == [str(i) for i in range(8)]
    assert all(e["LOCAL_RANK"] == e["RANK"] and e["WORLD_SIZE"] == "8" for e in envs)
    assert all(e["MASTER_ADDR"] == "127.0.0.1" and e["MASTER_PORT"] == "29511" for e in envs)
    assert all(e["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and e["SVIHMM_BENCH_CHILD"] == "1" for e in envs)
    # a caller's own setting of the IPC mode is respected
    assert bench.rank_envs(1, 1, base={"HSA_ENABLE_IPC_MODE_LEGACY": "1"})[0]["HSA_ENABLE_IPC_MODE_LEGACY"] == "1"


def test_failed_rank_zero_still_prints_one_json_line():
    """VERDICT r4 next #5b: a multi-rank run whose rank 0 cannot come up (here: its HIP library does not load,
    under a torchrun-style environment -- so also on a machine with a GPU, where rank 0 would otherwise wait
    for a peer that never starts) leaves the error record, not silence."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29999",
               SVIHMM_RENDEZVOUS_TIMEOUT="2", SVIHMM_HIP_LIB="/nonexistent/libsvihmm_hip.so")
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0
    lines = [l for l in p.stdout.splitlines() if l.lstrip().startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["value"] is None and rec["n_gpus"] == 2 and "error" in rec


def test_self_launch_refusal_prints_the_error_record():
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2"], env=env, capture_output=True,
                       text=True, timeout=120)
    rec = json.loads([l for l in p.stdout.splitlines() if l.lstrip().startswith("{")][-1])
    assert rec["value"] is None and "HIP device" in rec["error"]


def test_self_launch_without_the_built_library_prints_the_error_record():
    """first contact with a box whose libsvihmm_hip.so is missing (or does not load) -- the
    launcher's preamble raises before any rank exists; the ONE JSON line is still there."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["SVIHMM_HIP_LIB"] = "/nonexistent/libsvihmm_hip.so"
    for gpus in ("2", "1"):
        p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", gpus, "--steps", "1", "--warmup", "0"],
                           env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode != 0
        lines = [l for l in p.stdout.splitlines() if l.lstrip().startswith("{")]
        assert len(lines) == 1, p.stdout + p.stderr
        rec = json.loads(lines[0])
        assert rec["value"] is None and rec["n_gpus"] == int(gpus) and "error" in rec
