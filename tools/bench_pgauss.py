"""Timing of the Gaussian-tracks family (svihmm_set_emission_pgauss) on one MI355X; bench.py is not involved.

    python tools/bench_pgauss.py [--out profiles/pgauss_bench.json] [--limit 420]

Model: K = 64 states, D = 32 real-valued tracks (F = 96 statistics rows), column means about 1e3, spreads log-uniform
in [0.1, 10], 2 % of the entries missing (NaN).
Cases:
  windows    the bench geometry: T = 1e6 rows in 3891 windows of 257 rows, one estep_minibatch (TRANS_WRAP)
  sequences  4096 sequences of 32 .. 512 rows (about 1.1e6 rows), one estep_sequences
Routes:
  device     set_emission_pgauss (the tables change every iteration) + the one E-step call, statistics read back
  host       what a user does without the family: the contract's loop in NumPy (per column r = x - mu, r * r, * hprec,
             + cst over the present entries, 16384 rows at a time), set_lliks, an E-step with USE_HOST_LLIKS under a NIW
             family of the observations' width (its statistics GEMM runs, as it would), var_x read back,
             [sxx | sx | n] as three products with var_x in NumPy (BLAS).  `sequences`: one such call per sequence.
  diag       the second yardstick: the same rows with NOTHING missing under the existing DiagonalGaussian device family
             (set_emission_diag + the same E-step call): a feature GEMM on MFMA against this family's VALU lookup.
Every (case, route) runs in a child process of its own under a time limit and with at most 16 threads; the first
child that fails, faults or runs out of time ends the run -- nothing else is started on the device after it.
device / diag: three warm-up calls, then 300 timed calls (each ends with the statistics on the host): the median, the
quartiles and the extremes of their wall times, and in a separate pass the kernel time per profile slot from HIP
events.  host: one warm-up on a twentieth of the data, then three timed passes (seconds long each): their median."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

K, D = 64, 32
LM, NWIN = 257, 3891
HOST_REPEATS = 3
N_SEQ = 4096


def model(rng):
    """(factors (mu, nus, alphas, betas) [K, D], tables (mu, hprec, cst), means [K, D], sig [D], mod_init, ltran)."""
    import numpy as np
    from scipy.special import digamma
    base = 1e3 + rng.normal(size=D) * 20.0
    sig = np.exp(rng.uniform(np.log(0.1), np.log(10.0), size=D))
    means = base[None, :] + sig[None, :] * 0.5 * rng.normal(size=(K, D))
    nus = rng.uniform(1.0, 50.0, size=(K, D))
    alphas = rng.uniform(2.0, 20.0, size=(K, D))
    betas = alphas * (sig[None, :] * np.exp(0.2 * rng.normal(size=(K, D)))) ** 2
    tabs = (means.copy(), -0.5 * alphas / betas,
            -0.5 / nus - 0.5 * (np.log(betas) - digamma(alphas)) - 0.5 * np.log(2.0 * np.pi))
    vt = 1.0 + rng.random((K, K)) * 20 + 200 * np.eye(K)
    vi = rng.random(K) + 0.1
    return ((means, nus, alphas, betas), tabs, means, sig,
            digamma(vi) - digamma(vi.sum()), digamma(vt) - digamma(vt.sum(1))[:, None])


def host_lliks(x, mu, hprec, cst, chunk=16384):
    """The contract's loop, rows in chunks that stay in cache."""
    import numpy as np
    ll = np.empty((x.shape[0], mu.shape[0]))
    for a in range(0, x.shape[0], chunk):
        xc = x[a:a + chunk]
        with np.errstate(invalid="ignore"):
            ok = (xc > -1e150) & (xc < 1e150)
        s = np.zeros((xc.shape[0], mu.shape[0]))
        for d in range(xc.shape[1]):
            okd = ok[:, d]
            r = np.where(okd, xc[:, d], 0.0)[:, None] - mu[:, d][None, :]
            p = r * r
            p = p * hprec[:, d][None, :]
            t = s + p
            t = t + cst[:, d][None, :]
            s = np.where(okd[:, None], t, s)
        ll[a:a + chunk] = s
    return ll


def host_stats(x, q, origin):
    import numpy as np
    with np.errstate(invalid="ignore"):
        ok = (x > -1e150) & (x < 1e150)
    r = np.where(ok, x - origin[None, :], 0.0)
    return np.concatenate([q.T.dot(r * r), q.T.dot(r), q.T.dot(ok.astype(np.float64))], axis=1)


REPEATS = 300


def timed_ms(fn, n=REPEATS, warm=3):
    """Sorted wall times (ms) of n calls after the warm-up calls."""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts


def device_name():
    """Target and CU count of the first GPU node in the kernel driver's topology ("unknown" where there is none)."""
    import glob
    for node in sorted(glob.glob("/sys/class/kfd/kfd/topology/nodes/*")):
        try:
            props = dict(l.split()[:2] for l in open(os.path.join(node, "properties")) if len(l.split()) >= 2)
            if int(props.get("simd_count", "0")) > 0:
                v = int(props.get("gfx_target_version", "0"))       # 90500 = gfx950
                return "gfx%d%x%x, %d CUs" % (v // 10000, v // 100 % 100, v % 100,
                                              int(props["simd_count"]) // max(int(props.get("simd_per_cu", "4")), 1))
        except (OSError, ValueError, KeyError):
            continue
    return "unknown"


def run_child(case, route):
    import numpy as np
    from pysvihmm_amd import _lib as L
    from pysvihmm_amd.engine import HipEngine
    rng = np.random.default_rng(11)
    fac, tabs, means, sig, mod_init, ltran = model(rng)
    if case == "windows":
        T = NWIN * LM
        starts = np.arange(NWIN, dtype=np.int64) * LM
        lens = None
    else:
        lens = np.random.default_rng(20).integers(32, 513, size=N_SEQ).astype(np.int64)
        T = int(lens.sum())
    off = None if lens is None else np.concatenate(([0], np.cumsum(lens)))
    x = means[rng.integers(0, K, size=T)] + sig[None, :] * rng.normal(size=(T, D))
    if route != "diag":
        x[rng.random((T, D)) < 0.02] = np.nan
    with np.errstate(invalid="ignore"):
        origin = np.nanmean(x, axis=0)
    eng = HipEngine(0)
    if route == "device":
        eng.set_emission_pgauss(*tabs, origin=origin)       # (the rows are uploaded under the family: not centred)
    eng.set_obs(x, None)
    eng.set_globals(mod_init, ltran)
    out = {}
    res = {"case": case, "route": route, "K": K, "D": D, "F": 3 * D if route != "diag" else 2 * D + 1, "rows": T,
           "missing": 0.0 if route == "diag" else 0.02}
    if route in ("device", "diag"):
        def setter():
            if route == "device":
                eng.set_emission_pgauss(*tabs, origin=origin)
            else:
                eng.set_emission_diag(*fac, check=False)
        if lens is not None:
            setter()
            eng.set_sequences(lens)

        def call():
            setter()
            if lens is None:
                st = eng.estep(starts, LM, flags=L.TRANS_WRAP)
            else:
                st = eng.estep_sequences(flags=0)[0]
            out["counts"], out["lb"] = (st.flat if route == "device" else st.buf[K * K:-1]), float(st.lb[0])
        ts = timed_ms(call)
        med, lo, hi = ts[len(ts) // 2], ts[0], ts[-1]
        eng.profile(True)
        eng.profile_reset()
        call()
        pr = eng.profile_read()
        eng.profile(False)
        res.update(call_ms=med, call_ms_min=lo, call_ms_max=hi, call_ms_q1=ts[len(ts) // 4], call_ms_q3=ts[3 * len(ts) // 4],
                   repeats=len(ts), timed_window_s=sum(ts) / 1e3,
                   kernel_ms={k: round(v[0], 4) for k, v in pr.items() if v[1]},
                   launches={k: int(v[1]) for k, v in pr.items() if v[1]})
    else:
        eng.set_emission_niw(np.full((K, D), 0.5), np.stack([np.eye(D)] * K), np.ones(K), np.full(K, D + 2.0))
        wins = [(0, T)] if lens is None else [(int(off[s]), int(lens[s])) for s in range(N_SEQ)]

        def one(a, n, st0, lm):
            ll = host_lliks(x[a:a + n], *tabs)
            eng.set_lliks(ll.reshape(len(st0), lm, K))
            st = eng.estep(st0, lm, flags=L.USE_HOST_LLIKS | (L.TRANS_WRAP if lens is None else 0))
            q = eng.read_intermediate("var_x", len(st0), lm).reshape(n, K)
            return host_stats(x[a:a + n], q, origin), float(st.lb[0])

        def sweep(ws):
            counts, lb = 0.0, 0.0
            for a, n in ws:
                if lens is None:
                    c, l = one(a, n, starts[:n // LM], LM)
                else:
                    c, l = one(a, n, np.array([a], dtype=np.int64), n)
                counts, lb = counts + c, lb + l
            return counts, lb
        sweep([(0, (NWIN // 20) * LM)] if lens is None else wins[:N_SEQ // 20])
        ts = []
        for _ in range(HOST_REPEATS):
            t0 = time.perf_counter()
            out["counts"], out["lb"] = sweep(wins)
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        res.update(call_ms=ts[len(ts) // 2], call_ms_min=ts[0], call_ms_max=ts[-1], repeats=len(ts))
    assert np.all(np.isfinite(out["counts"]))
    res.update(lb=out["lb"], counts_total=float(np.sum(out["counts"])))
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["windows", "sequences"])
    ap.add_argument("--route", choices=["device", "host", "diag"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=420)
    args = ap.parse_args()
    if args.case:
        run_child(args.case, args.route)
        return 0
    env = dict(os.environ)
    for var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):       # at most 16 threads a child
        try:
            env[var] = str(max(1, min(int(env.get(var, "16")), 16)))
        except ValueError:
            env[var] = "16"
    if not os.path.exists("/dev/kfd"):
        print("bench_pgauss: no GPU (a time is only a time on the device)", file=sys.stderr)
        return 2
    results, rc = [], 0
    for case in ("windows", "sequences"):
        for route in ("device", "diag", "host"):
            tag = {"case": case, "route": route}
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--route", route], cwd=REPO,
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.limit, text=True, env=env)
            except subprocess.TimeoutExpired:
                results.append(dict(tag, error="time limit of %d s" % args.limit))
                rc = 1
                break
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                results.append(dict(tag, error="exit status %d" % p.returncode, stderr=p.stderr[-2000:]))
                rc = 1
                break          # nothing more on the device after a failure
            results.append(json.loads(line[-1][7:]))
            print(json.dumps(results[-1]), flush=True)
        if rc:
            break
    summary = {}
    for case in ("windows", "sequences"):
        r = {x["route"]: x for x in results if x.get("case") == case and "call_ms" in x}
        if "device" in r and "host" in r:
            summary[case] = {"device_ms": r["device"]["call_ms"], "device_ms_quartiles": [r["device"]["call_ms_q1"], r["device"]["call_ms_q3"]],
                             "host_ms": r["host"]["call_ms"],
                             "host_over_device": r["host"]["call_ms"] / r["device"]["call_ms"],
                             "device_kernel_ms": r["device"]["kernel_ms"],
                             "lb_rel_diff": abs(r["device"]["lb"] - r["host"]["lb"]) / abs(r["host"]["lb"]),
                             "stats_total_rel_diff": abs(r["device"]["counts_total"] - r["host"]["counts_total"])
                             / abs(r["host"]["counts_total"])}
            if "diag" in r:
                summary[case].update(diag_complete_data_ms=r["diag"]["call_ms"], diag_kernel_ms=r["diag"]["kernel_ms"],
                                     device_over_diag=r["device"]["call_ms"] / r["diag"]["call_ms"])
    doc = {"tool": "tools/bench_pgauss.py", "device": device_name(), "summary": summary, "results": results}
    print(json.dumps({"summary": summary}), flush=True)
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
