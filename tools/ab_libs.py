"""A/B of experiment builds on one box: per-kernel HIP-event times of the bench E-step for
each library given on the command line (run one process per library: SVIHMM_HIP_LIB); with --bench, alternating
fresh bench.py processes per library and the acceptance figures (see below)."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import sys, os
sys.path.insert(0, %r)
import numpy as np
import bench
from pysvihmm_amd.engine import HipEngine
from pysvihmm_amd import _lib as L
sys.path.insert(0, os.path.join(%r, "tools"))
from _workload import bench_problem
e = HipEngine(0)
pb = bench_problem(e)
B = bench.T // bench.LM
st = np.arange(B, dtype=np.int64) * bench.LM
e.set_globals(pb["mod_init"], pb["ltran"]); e.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
for _ in range(3): e.estep(st, bench.LM, flags=L.TRANS_WRAP, read=False)
e.sync(); e.profile(True); e.profile_reset()
for _ in range(10): e.estep(st, bench.LM, flags=L.TRANS_WRAP, read=False)
p = e.profile_read()
print({k: round(v[0] / max(v[1], 1), 4) for k, v in p.items() if v[1]})
''' % (ROOT, ROOT)
# --bench N [--json FILE] [--s64] lib lib ...: N alternating rounds of fresh `bench.py --full --no-side --no-cpu-baseline`
# processes, one per library and round -- ms_per_step and the statistics slot's HIP-event time of every run, the
# acceptance figures of DESIGN 4 for the LAST library against the FIRST (every run below every run of the first; median
# difference against the first's standard deviation); --s64: the 64-window minibatch step of each library and round as well.
# A library is "base" (the product) or a path relative to the repository.
CHILD64 = r'''
import sys, os, time
sys.path.insert(0, %r)
import numpy as np
import bench
from pysvihmm_amd.engine import HipEngine
from pysvihmm_amd import _lib as L
sys.path.insert(0, os.path.join(%r, "tools"))
from _workload import bench_problem
e = HipEngine(0)
pb = bench_problem(e)
st = (np.arange(64, dtype=np.int64) * (bench.T // 64)) %% (bench.T - bench.LM)
def step():
    e.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"], check=False)
    e.set_globals(pb["mod_init"], pb["ltran"])
    e.estep(st, bench.LM, flags=L.TRANS_WRAP, read=False)
    return e.read_packed()
for _ in range(5): step()
bl = []
for _ in range(7):
    e.sync(); t0 = time.perf_counter()
    for _ in range(40): step()
    e.sync(); bl.append((time.perf_counter() - t0) / 40 * 1e3)
print(round(float(np.median(bl)), 5))
''' % (ROOT, ROOT)


def lib_env(lib):
    env = dict(os.environ)
    if lib != "base":
        env["SVIHMM_HIP_LIB"] = os.path.join(ROOT, lib)
    return env


def bench_ab(argv):
    import json
    import statistics
    n = int(argv[argv.index("--bench") + 1])
    out_json = argv[argv.index("--json") + 1] if "--json" in argv else None
    skip = {argv.index("--bench") + 1} | ({argv.index("--json") + 1} if out_json else set())
    libs = [a for i, a in enumerate(argv) if not a.startswith("--") and i not in skip]
    runs = {lib: {"ms_per_step": [], "stats_ms": [], "kernel": None} for lib in libs}
    for rnd in range(n):
        for lib in libs:
            cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--no-side", "--no-cpu-baseline"]
            out = subprocess.run(cmd, env=lib_env(lib), capture_output=True, text=True)
            if out.returncode:
                sys.exit("bench.py failed for %s (rc %d): %s" % (lib, out.returncode, out.stderr[-600:]))
            r = json.loads(out.stdout.strip().splitlines()[-1])
            runs[lib]["ms_per_step"].append(r["ms_per_step"])
            runs[lib]["stats_ms"].append(r["kernels"]["stats"]["ms_per_launch"])
            runs[lib]["kernel"] = r["roofline"].get("kernel_function")
            print(rnd, lib, "ms_per_step %.4f stats %.4f" % (r["ms_per_step"], r["kernels"]["stats"]["ms_per_launch"]), flush=True)
            if "--s64" in argv:
                o = subprocess.run([sys.executable, "-c", CHILD64], env=lib_env(lib), capture_output=True, text=True)
                if o.returncode:
                    sys.exit("minibatch child failed for %s: %s" % (lib, o.stderr[-600:]))
                runs[lib].setdefault("minibatch_s64_ms", []).append(float(o.stdout.strip().splitlines()[-1]))
                print(rnd, lib, "minibatch_s64 ms_per_step", runs[lib]["minibatch_s64_ms"][-1], flush=True)
    res = {"command": "bench.py --full --no-side --no-cpu-baseline, %d alternating rounds of fresh processes" % n,
           "runs": runs}
    a, b = runs[libs[0]], runs[libs[-1]]
    for key in ("ms_per_step", "stats_ms") + (("minibatch_s64_ms",) if "--s64" in argv else ()):
        sd = statistics.stdev(a[key]) if n > 1 else float("nan")
        diff = statistics.median(a[key]) - statistics.median(b[key])
        res["verdict_" + key] = {"first": libs[0], "last": libs[-1], "median_first": statistics.median(a[key]),
                                 "median_last": statistics.median(b[key]), "median_difference": diff,
                                 "stdev_first": sd, "difference_over_stdev": diff / sd if sd else None,
                                 "every_last_below_every_first": max(b[key]) < min(a[key])}
        print(key, res["verdict_" + key])
    if out_json:
        with open(out_json, "w") as f:
            json.dump(res, f, indent=1)


if "--bench" in sys.argv:
    bench_ab(sys.argv[1:])
    sys.exit(0)
for rnd in range(2):
    for lib in sys.argv[1:]:
        out = subprocess.run([sys.executable, "-c", CHILD], env=lib_env(lib), capture_output=True, text=True)
        print(rnd, lib, out.stdout.strip().splitlines()[-1] if out.stdout.strip() else out.stderr[-400:])
