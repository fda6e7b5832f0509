"""Timing of entry-wise held-out scoring (svihmm_heldout_entries) on one MI355X; bench.py is not involved.

    python tools/bench_heldout.py [--out profiles/heldout_bench.json] [--limit 540]

Model: K = 64 states, D = 32 Poisson count tracks, rates log-uniform in [0.05, 200], counts up to 4095; 5 % of the
entries are held out (blanked -- NaN -- in the resident copy, their values kept in the entry list).
Cases:
  chain      T = 1e6 rows as one chain: one forward_backward over [0, T), then the held-out entries
  sequences  4096 sequences of 32 .. 512 rows (about 1.1e6 rows): one estep_sequences, then the held-out entries
Routes, alternating in ONE process per case (device, host, device, host, ...), the median of each reported:
  device     the E-step call + heldout_entries(rows, cols, vals): two doubles come back
  host       the same E-step call + read_rows("var_x", 0, T) + the same formula in NumPy
             (LSE_k(log(q[row] + 1e-9) + c elog - erate - logfact[c]), in pieces of 131072 entries)
One warm-up round of both routes, then 7 timed rounds.  Separately (profiling on, after the timed rounds) the
held-out kernels' own time from HIP events, against the bytes they must move -- n (8 K + 20) in, 16 K D of table
pairs, 8 (C + 1) of logfact -- as a share of the 8 TB/s of the data sheet.  The E-step's own time is reported too, so
that the scoring step's cost is visible on its own.  Each case runs in a child process under a time limit; a child
that fails ends the run."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

K, D = 64, 32
CMAX = 4095
FRAC = 0.05
N_SEQ = 4096
ROUNDS = 7
PIECE = 131072
HBM_PEAK = 8.0e12


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def host_entries(q, rows, cols, vals, elog, erate, logfact):
    import numpy as np
    tot, n = 0.0, 0
    for a in range(0, len(rows), PIECE):
        r, c, v = rows[a:a + PIECE], cols[a:a + PIECE], vals[a:a + PIECE]
        ci = v.astype(np.int64)
        t = v[:, None] * elog[:, c].T - erate[:, c].T - logfact[ci][:, None]
        s = np.log(q[r] + 1e-9) + t
        m = s.max(1)
        tot += float(np.sum(m + np.log(np.exp(s - m[:, None]).sum(1))))
        n += len(r)
    return tot / n, n


def run_child(case):
    import numpy as np
    from scipy.special import digamma, gammaln
    from pysvihmm_amd import _lib as L
    from pysvihmm_amd import util
    from pysvihmm_amd.engine import HipEngine
    rng = np.random.default_rng(11)
    base = np.exp(rng.uniform(np.log(0.05), np.log(200.0), size=D))
    lam = base[None, :] * np.exp(0.3 * rng.normal(size=(K, D)))
    b = rng.uniform(0.5, 20.0, size=(K, D))
    a = lam * b
    elog, erate = digamma(a) - np.log(b), a / b
    logfact = gammaln(np.arange(CMAX + 1.0) + 1.0)
    vt = 1.0 + rng.random((K, K)) * 20 + 200 * np.eye(K)
    vi = rng.random(K) + 0.1
    mod_init, ltran = digamma(vi) - digamma(vi.sum()), digamma(vt) - digamma(vt.sum(1))[:, None]
    if case == "chain":
        T, lens = 1000000, None
    else:
        lens = np.random.default_rng(20).integers(32, 513, size=N_SEQ).astype(np.int64)
        T = int(lens.sum())
    x = np.minimum(rng.poisson(lam[rng.integers(0, K, size=T)]), CMAX).astype(np.float64)
    xb, rows, cols, vals = util.speckle_holdout(x, FRAC, seed=3)
    eng = HipEngine(0)
    eng.set_obs(xb, None)
    eng.set_globals(mod_init, ltran)
    eng.set_emission_poisson(elog, erate, CMAX)
    if lens is not None:
        eng.set_sequences(lens)

    def estep():
        if lens is None:
            eng.forward_backward([0], T, flags=0, want=())
        else:
            eng.estep_sequences(flags=0, read=False)

    def device():
        estep()
        return eng.heldout_entries(rows, cols, vals, resident=False)

    def host():
        estep()
        return host_entries(eng.read_rows("var_x", 0, T), rows, cols, vals, elog, erate, logfact)

    def only_estep():
        estep()
        eng.sync()

    out = {}
    times = {"device": [], "host": [], "estep": []}
    for rnd in range(ROUNDS + 1):
        for name, fn in (("device", device), ("host", host), ("estep", only_estep)):
            t0 = time.perf_counter()
            out[name] = fn()
            if rnd:                               # round 0 warms every shape up
                times[name].append((time.perf_counter() - t0) * 1e3)
    # the held-out kernels' own time: HIP events around the launches, a pass of its own
    estep()
    eng.sync()
    eng.profile(True)
    kern = []
    for _ in range(20):
        eng.profile_reset()
        eng.heldout_entries(rows, cols, vals, resident=False)
        kern.append(eng.profile_read()["misc"][0])
    eng.profile(False)
    n = len(rows)
    bytes_in = n * (8 * K + 20) + 16 * K * D + 8 * (CMAX + 1)
    kms = median(kern)
    res = {"case": case, "K": K, "D": D, "rows": T, "entries": n, "rounds": ROUNDS,
           "device_ms": median(times["device"]), "device_ms_all": [round(t, 3) for t in times["device"]],
           "host_ms": median(times["host"]), "host_ms_all": [round(t, 1) for t in times["host"]],
           "estep_ms": median(times["estep"]),
           "host_over_device": median(times["host"]) / median(times["device"]),
           "heldout_kernels_ms": kms, "heldout_kernels_ms_min_max": [min(kern), max(kern)],
           "bytes_must_move": bytes_in, "share_of_8TBs": bytes_in / (kms * 1e-3) / HBM_PEAK,
           "mean_device": out["device"][0], "mean_host": out["host"][0],
           "mean_rel_diff": abs(out["device"][0] - out["host"][0]) / abs(out["host"][0]),
           "count": out["device"][1]}
    assert out["device"][1] == out["host"][1] == n
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
        print("bench_heldout: no GPU (a time is only a time on the device)", file=sys.stderr)
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
    doc = {"tool": "tools/bench_heldout.py", "results": results}
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
