"""Timing of svihmm_ffbs_windows (Engine.ffbs_windows) on one MI355X; bench.py is not involved.

    python tools/bench_ffbs_windows.py [--out profiles/ffbs_windows_bench.json] [--limit 300]

Every case runs in a child process of its own under a time limit (``--limit`` seconds); the first case
that fails, faults or runs out of time ends the run -- nothing else is started on the device after it.
The model is bench.py's (K=64, D=32, T=1e6, sequence generated in HBM); the draws use the device's
counter-based uniforms (nothing is uploaded), logA = the filter's ltran.  Cases:
  windows64   64 windows x 257 rows, S = 1 and S = 64
  epoch       the epoch batch, 3891 windows x 257 rows, S = 1
  chain       the whole chain B = 1, Lm = T: S = 1 and S = 16 from one filter, and -- the baseline, in the same
              process, alternating with the S = 16 call -- the same 16 draws as 16 calls of svihmm_ffbs
              (each re-runs the filter and uploads its T uniforms)
Per entry: wall time of the whole call (median of the repeats after warm-up calls of the same shape; the
call ends in a stream synchronisation and includes the read-back of z) and, from HIP events in a separate
call, the kernel time of the phases (emission, forward filter, backward sampling)."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

CASES = ["windows64", "epoch", "chain"]


def stats(ts):
    ts = sorted(ts)
    return {"call_ms": ts[len(ts) // 2], "call_ms_min": ts[0], "call_ms_max": ts[-1], "repeats": len(ts)}


def timed_calls(fns, reps, warm=2):
    """Median wall time of each callable, the callables alternating inside every repeat."""
    for _ in range(warm):
        for fn in fns:
            fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[i].append((time.perf_counter() - t0) * 1e3)
    return [stats(t) for t in ts]


def phases(eng, fn):
    eng.profile(True)
    eng.profile_reset()
    fn()
    pr = eng.profile_read()
    eng.profile(False)
    return {"emission_kernel_ms": pr.get("emission", (0.0, 0))[0], "filter_kernels_ms": pr.get("forward_backward", (0.0, 0))[0],
            "sampling_kernels_ms": pr.get("ffbs_sample", (0.0, 0))[0], "d2h_ms": pr.get("d2h", (0.0, 0))[0]}


def windows_entry(eng, starts, Lm, logA, S, reps):
    import numpy as np
    out = {}

    def call():
        out["z"] = eng.ffbs_windows(starts, Lm, logA, n_draws=S, seed=12345)[0]
    rec = {"B": int(len(starts)), "Lm": int(Lm), "S": int(S), "K": int(eng.K)}
    rec.update(timed_calls([call], reps)[0])
    rec.update(phases(eng, call))
    z = out["z"]
    assert z.shape == (S, len(starts), Lm) and z.min() >= 0 and z.max() < eng.K
    rec["distinct_paths"] = int(len(np.unique(z.reshape(S, -1), axis=0)))
    return rec


def run_case(name):
    import numpy as np
    import bench
    from _workload import bench_problem
    from pysvihmm_amd.engine import HipEngine
    eng = HipEngine(0)
    pb = bench_problem(eng)
    eng.set_globals(pb["mod_init"], pb["ltran"])
    eng.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
    K, T, LM = bench.K, bench.T, bench.LM
    logA = np.ascontiguousarray(pb["ltran"])
    res = {"case": name, "K": K, "D": bench.D, "T": T}
    if name == "windows64":
        st = (np.arange(64, dtype=np.int64) * (T // 64)) // LM * LM
        res["entries"] = [windows_entry(eng, st, LM, logA, S, 20) for S in (1, 64)]
    elif name == "epoch":
        st = np.arange(T // LM, dtype=np.int64) * LM
        res["entries"] = [windows_entry(eng, st, LM, logA, 1, 10)]
    else:
        res["entries"] = [windows_entry(eng, [0], T, logA, 1, 5)]
        S = 16
        rs = np.random.RandomState(7)
        u = rs.random_sample((S, 1, T))
        out = {}

        def one_filter():
            out["zw"] = eng.ffbs_windows([0], T, logA, n_draws=S, uniforms=u)[0]

        def sixteen_calls():
            out["zf"] = [eng.ffbs(logA, u[s, 0], want_lalpha=False)[0] for s in range(S)]
        a, b = timed_calls([one_filter, sixteen_calls], 5, warm=1)
        ea = {"B": 1, "Lm": T, "S": S, "K": K, "what": "svihmm_ffbs_windows, S = 16, host uniforms"}
        ea.update(a)
        ea.update(phases(eng, one_filter))
        eb = {"B": 1, "Lm": T, "S": S, "K": K, "what": "16 calls of svihmm_ffbs (baseline)"}
        eb.update(b)
        eb.update(phases(eng, sixteen_calls))
        same = all(np.array_equal(out["zw"][s, 0], out["zf"][s]) for s in range(S))
        res["same_paths_as_baseline"] = bool(same)
        res["entries"] += [ea, eb]
        res["entries"].append(windows_entry(eng, [0], T, logA, S, 5))          # device uniforms: nothing uploaded
        res["speedup_one_filter_vs_16_calls"] = b["call_ms"] / a["call_ms"]
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=300)
    args = ap.parse_args()
    if args.case:
        run_case(args.case)
        return 0
    if not os.path.exists("/dev/kfd"):
        print("bench_ffbs_windows: no GPU (a time is only a time on the device)", file=sys.stderr)
        return 2
    results = []
    rc = 0
    for case in CASES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case], cwd=REPO,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.limit, text=True)
        except subprocess.TimeoutExpired:
            results.append({"case": case, "error": "time limit of %d s" % args.limit})
            rc = 1
            break
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            results.append({"case": case, "error": "exit status %d" % p.returncode, "stderr": p.stderr[-2000:]})
            rc = 1
            break          # nothing more on the device after a failure
        results.append(json.loads(line[-1][7:]))
        print(json.dumps(results[-1]), flush=True)
    doc = {"tool": "tools/bench_ffbs_windows.py", "device": "MI355X", "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    if rc:
        print(json.dumps(results[-1]), file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
