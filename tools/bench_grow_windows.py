"""Timing of one adaptive selection (VBHMM.select_buffer / select_L) on one MI355X: the device route
(svihmm_grow_windows, one call) against the host-driven route (``device_growth = False``: one device
E-step and one read-back per candidate half-width); bench.py is not involved.

    python tools/bench_grow_windows.py [--out profiles/grow_windows_bench.json] [--limit 600]

One handle, the bench workload's shape (BASELINE configs[2]: K = 64, D = 32, T = 1e6), n = 64 centres.
Three variational states: ``bench`` (var_tran = 1 + U(0,1) T/K, the timed E-step's state), ``sticky``
(var_tran = 1 + 200 I + U(0,1)) -- with the bench workload's well-separated emissions both stop after one
candidate -- and ``sticky_weak`` (the sticky transitions with every sigma_mf scaled by 1000, a weak sticky
model as in the growth tests: several candidates).  Selections: ``select_buffer(halfL=128)`` and ``select_L(minHalfL=1)``.
Method (the measuring guide's): both routes alternate inside one process with the same seed before every
call (same centres), two warm-up rounds, then the median over the repeats of the wall time of the whole
call (each ends in a stream synchronisation).  A separate profiled pass splits the device route into its
emission pass and its growth launch (HIP events), and one call of the engine with a trace buffer gives
the steps taken; the product kernel's time per growth row is the growth launch over the rows the longest
centre adds (prologue rows included: 2 m for Mid, half0 - m, then increment per step).
The work runs in a child process under a time limit; nothing else is started on the device after a
failure."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

N_CENTRES, REPEATS, WARM = 64, 9, 2


def build_model(eng):
    import numpy as np
    import bench
    from _workload import bench_problem
    from pysvihmm_amd import hmmsgd_metaobs
    from pysvihmm_amd.distributions import Gaussian
    pb = bench_problem(eng, want_obs=True)
    K, D = bench.K, bench.D
    emit = []
    for k in range(K):
        e = Gaussian(mu=pb["mu"][k], sigma=np.eye(D), mu_0=np.zeros(D), sigma_0=pb["sigma0"], kappa_0=0.01, nu_0=D + 2.0)
        e.mu_mf, e.sigma_mf = pb["mu"][k].copy(), pb["sigma"][k].copy()
        e.kappa_mf, e.nu_mf = float(pb["kappa"][k]), float(pb["nu"][k])
        emit.append(e)
    hmm = hmmsgd_metaobs.VBHMM(pb["obs"], np.ones(K), np.ones((K, K)), np.array(emit), metaobs_half=bench.LHALF,
                               mb_sz=N_CENTRES, maxit=1, seed=bench.SEED, engine=eng)
    rs = np.random.RandomState(bench.SEED + 7)
    sticky = 1.0 + 200.0 * np.eye(K) + rs.random_sample((K, K))
    states = {"bench": (1.0 + rs.random_sample((K, K)) * bench.T / K, 1.0), "sticky": (sticky, 1.0),
              "sticky_weak": (sticky, 1000.0)}
    return hmm, states, pb["sigma"]


def median_pair(hmm, name, kw, seed):
    """Alternating device / host route, same centres: medians (ms) and the two answers."""
    import numpy as np
    ts = {True: [], False: []}
    ans = {}
    for r in range(WARM + REPEATS):
        for dev in (True, False):
            hmm.device_growth = dev
            np.random.seed(seed)
            t0 = time.perf_counter()
            ans[dev] = getattr(hmm, name)(**kw)
            dt = (time.perf_counter() - t0) * 1e3
            if r >= WARM:
                ts[dev].append(dt)
    hmm.device_growth = True
    med = lambda v: sorted(v)[len(v) // 2]
    return {"device_ms": med(ts[True]), "device_ms_min": min(ts[True]), "device_ms_max": max(ts[True]),
            "host_ms": med(ts[False]), "host_ms_min": min(ts[False]), "host_ms_max": max(ts[False]),
            "device_result": int(ans[True]), "host_result": int(ans[False]), "repeats": REPEATS}


def run():
    import numpy as np
    from pysvihmm_amd.engine import HipEngine
    eng = HipEngine(0)
    hmm, states, sigma = build_model(eng)
    T = hmm.T
    out = []
    sels = [("select_buffer", dict(numIndices=N_CENTRES, halfL=128), 128, 128),
            ("select_L", dict(numIndices=N_CENTRES, minHalfL=1), 1, 0)]
    for sname, (vt, sigma_scale) in states.items():
        hmm.var_tran = vt.copy()
        for k, e in enumerate(hmm.var_emit):
            e.sigma_mf = sigma[k] * sigma_scale
        for name, kw, half0, m in sels:
            seed = 4242
            rec = {"state": sname, "selection": name, "n": N_CENTRES, "half0": half0, "probe_off": m,
                   "K": hmm.K, "D": hmm.D, "T": int(T)}
            rec.update(median_pair(hmm, name, kw, seed))
            # steps taken and the split of the device route, on the centres the timed calls drew
            np.random.seed(seed)
            centres = np.random.choice(T - 2 * half0 - 1, size=N_CENTRES) + half0
            half, steps, _ = eng.grow_windows(centres, half0, probe_off=m)
            rec["steps_min"], rec["steps_max"] = int(steps.min()), int(steps.max())
            rec["steps_mean"] = float(steps.mean())
            rec["half_max"] = int(half.max())
            assert rec["half_max"] == rec["device_result"] == rec["host_result"]
            eng.profile(True)
            eng.profile_reset()
            eng.grow_windows(centres, half0, probe_off=m)
            pr = eng.profile_read()
            eng.profile(False)
            rec["emission_pass_ms"] = pr.get("emission", (0.0, 0))[0]
            rec["growth_launch_ms"] = pr.get("forward_backward", (0.0, 0))[0]
            rows = 2 * m + (half0 - m) + int(steps.max())       # products of the longest centre, per side
            rec["growth_rows_longest_centre"] = rows
            rec["us_per_growth_row"] = rec["growth_launch_ms"] * 1e3 / max(rows, 1)
            out.append(rec)
            print(json.dumps(rec), flush=True)
    eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=600)
    args = ap.parse_args()
    if args.child:
        run()
        return 0
    if not os.path.exists("/dev/kfd"):
        print("bench_grow_windows: no GPU (a time is only a time on the device)", file=sys.stderr)
        return 2
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], cwd=REPO,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.limit, text=True)
    except subprocess.TimeoutExpired:
        print("bench_grow_windows: time limit of %d s" % args.limit, file=sys.stderr)
        return 1
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        print(p.stdout[-2000:], file=sys.stderr)
        print(p.stderr[-2000:], file=sys.stderr)
        return 1
    doc = {"tool": "tools/bench_grow_windows.py", "device": "MI355X", "results": json.loads(line[-1][7:])}
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
