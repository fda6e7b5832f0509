"""Timing of posterior expectations of per-state tables (svihmm_posterior_expect / _entries) on one MI355X; bench.py is
not involved.

    python tools/bench_posterior_expect.py [--out profiles/posterior_expect_bench.json] [--limit 540]

Model: K = 64 states; the posterior rows come from one E-step of a Poisson model on 8 count tracks (the calls do not
depend on the family: any E-step leaves rows to average).  Tables: F = 32 (state means) and F = 64 ([m | m^2 + s]),
entries about 1e2.
Cases:
  chain      T = 1e6 rows as one chain: one forward_backward over [0, T), then the calls against the batch held
  sequences  4096 sequences of 32 .. 512 rows (about 1.1e6 rows): one estep_sequences, then the calls
Routes, alternating in ONE process per case (device, host, device, host, ...), the median of each reported:
  device     posterior_expect(table): [rows, F] comes back / posterior_expect_entries on 2 % of the [rows, 32] entries
  host       read_rows("var_x", 0, rows) + the NumPy product (var_x @ table / the gathered rows' products, in pieces of
             131072 entries)
One warm-up round of every route, then 7 timed rounds.  Separately (profiling on, after the timed rounds) the dense
kernel's own time from HIP events, against the bytes it must move -- rows (K + F) 8 -- as a share of the 8 TB/s of
the data sheet: recorded, not gated.  Each case runs in a child process under a time limit; a child that fails ends
the run."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

K, D = 64, 8
CMAX = 4095
FS = (32, 64)
FRAC = 0.02
N_SEQ = 4096
ROUNDS = 7
PIECE = 131072
HBM_PEAK = 8.0e12


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def host_entries(q, tab, rows, cols):
    import numpy as np
    out = np.empty(len(rows))
    for a in range(0, len(rows), PIECE):
        r, c = rows[a:a + PIECE], cols[a:a + PIECE]
        out[a:a + PIECE] = np.einsum("ek,ke->e", q[r], tab[:, c])
    return out


def run_child(case):
    import numpy as np
    from scipy.special import digamma
    from pysvihmm_amd.engine import HipEngine
    rng = np.random.default_rng(11)
    base = np.exp(rng.uniform(np.log(0.05), np.log(200.0), size=D))
    lam = base[None, :] * np.exp(0.3 * rng.normal(size=(K, D)))
    b = rng.uniform(0.5, 20.0, size=(K, D))
    a = lam * b
    elog, erate = digamma(a) - np.log(b), a / b
    vt = 1.0 + rng.random((K, K)) * 20 + 200 * np.eye(K)
    vi = rng.random(K) + 0.1
    mod_init, ltran = digamma(vi) - digamma(vi.sum()), digamma(vt) - digamma(vt.sum(1))[:, None]
    if case == "chain":
        T, lens = 1000000, None
    else:
        lens = np.random.default_rng(20).integers(32, 513, size=N_SEQ).astype(np.int64)
        T = int(lens.sum())
    x = np.minimum(rng.poisson(lam[rng.integers(0, K, size=T)]), CMAX).astype(np.float64)
    eng = HipEngine(0)
    eng.set_obs(x, None)
    eng.set_globals(mod_init, ltran)
    eng.set_emission_poisson(elog, erate, CMAX)
    if lens is None:
        eng.forward_backward([0], T, flags=0, want=())
    else:
        eng.set_sequences(lens)
        eng.estep_sequences(flags=0, read=False)
    eng.sync()
    tabs = {F: 1e2 * rng.normal(size=(K, F)) for F in FS}
    n = int(FRAC * T * FS[0])
    rows = rng.integers(0, T, size=n)
    cols = rng.integers(0, FS[0], size=n).astype(np.int32)

    routes = []
    for F in FS:
        routes.append(("device_F%d" % F, lambda F=F: eng.posterior_expect(tabs[F])))
        routes.append(("host_F%d" % F, lambda F=F: eng.read_rows("var_x", 0, T) @ tabs[F]))
    routes.append(("device_entries", lambda: eng.posterior_expect_entries(tabs[FS[0]], rows, cols)))
    routes.append(("host_entries", lambda: host_entries(eng.read_rows("var_x", 0, T), tabs[FS[0]], rows, cols)))
    out = {}
    times = {name: [] for name, _ in routes}
    for rnd in range(ROUNDS + 1):
        for name, fn in routes:
            t0 = time.perf_counter()
            out[name] = fn()
            if rnd:                               # round 0 warms every shape up
                times[name].append((time.perf_counter() - t0) * 1e3)
    # the kernels' own time: HIP events around the launches, a pass of its own
    eng.profile(True)
    kern = {}
    for name, fn in [r for r in routes if r[0].startswith("device")]:
        ts = []
        for _ in range(10):
            eng.profile_reset()
            fn()
            ts.append(eng.profile_read()["misc"][0])
        kern[name] = ts
    eng.profile(False)
    res = {"case": case, "K": K, "rows": T, "rounds": ROUNDS, "entries": n}
    for F in FS:
        d, h = "device_F%d" % F, "host_F%d" % F
        must = T * (K + F) * 8
        kms = median(kern[d])
        scale = np.abs(out[h]).max()
        res["F%d" % F] = {"device_ms": median(times[d]), "device_ms_all": [round(t, 2) for t in times[d]],
                          "host_ms": median(times[h]), "host_ms_all": [round(t, 1) for t in times[h]],
                          "host_over_device": median(times[h]) / median(times[d]),
                          "kernel_ms": kms, "kernel_ms_min_max": [min(kern[d]), max(kern[d])],
                          "bytes_must_move": must, "share_of_8TBs": must / (kms * 1e-3) / HBM_PEAK,
                          "result_bytes": T * F * 8, "host_route_reads_bytes": T * K * 8,
                          "max_abs_diff_over_scale": float(np.abs(out[d] - out[h]).max() / scale)}
    d, h = "device_entries", "host_entries"
    res["entries_F%d" % FS[0]] = {"device_ms": median(times[d]), "device_ms_all": [round(t, 2) for t in times[d]],
                                  "host_ms": median(times[h]), "host_ms_all": [round(t, 1) for t in times[h]],
                                  "host_over_device": median(times[h]) / median(times[d]),
                                  "kernel_ms": median(kern[d]),
                                  "max_abs_diff_over_scale": float(np.abs(out[d] - out[h]).max() / np.abs(out[h]).max())}
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["chain", "sequences"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=540)
    args = ap.parse_args()
    if args.case:
        run_child(args.case)
        return 0
    if not os.path.exists("/dev/kfd"):
        print("bench_posterior_expect: no GPU (a time is only a time on the device)", file=sys.stderr)
        return 2
    env = dict(os.environ)
    for var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):       # at most 16 threads a child
        try:
            env[var] = str(max(1, min(int(env.get(var, "16")), 16)))
        except ValueError:
            env[var] = "16"
    results, rc = [], 0
    for case in ("chain", "sequences"):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case], cwd=REPO,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.limit, text=True, env=env)
        except subprocess.TimeoutExpired:
            results.append({"case": case, "error": "time limit of %d s" % args.limit})
            rc = 1
            break
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            results.append({"case": case, "error": "exit status %d" % p.returncode, "stderr": p.stderr[-2000:]})
            rc = 1
            break              # nothing more on the device after a failure
        results.append(json.loads(line[-1][7:]))
        print(json.dumps(results[-1]), flush=True)
    doc = {"tool": "tools/bench_posterior_expect.py", "results": results}
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
