"""Timing of the Poisson count family (svihmm_set_emission_poisson) on one MI355X; bench.py is not involved.

    python tools/bench_poisson.py [--out profiles/poisson_bench.json] [--limit 420]

Model: K = 64 states, D = 32 count tracks (F = 64 statistics rows), rates log-uniform in [0.05, 200], 2 % of the
entries missing, counts up to 4095.
Cases:
  windows    the bench geometry: T = 1e6 rows in 3891 windows of 257 rows, one estep_minibatch (TRANS_WRAP)
  sequences  4096 sequences of 32 .. 512 rows (about 1.1e6 rows), one estep_sequences
Routes:
  device     set_emission_poisson (the tables change every iteration) + the one E-step call, statistics read back
  host       what a user does without the family: NumPy lliks (c * elog - erate per column, gammaln table), set_lliks,
             an E-step with USE_HOST_LLIKS under a NIW family of the observations' width (its statistics GEMM runs, as
             it would), var_x read back, [sx | n] as two products with var_x in NumPy (BLAS).  `sequences`: one such
             call per sequence.
Every (case, route) runs in a child process of its own under a time limit and with at most 16 threads; the first
child that fails, faults or runs out of time ends the run -- nothing else is started on the device after it.
device: three warm-up calls, then 300 timed calls (each ends with the statistics on the host): the median, the
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
CMAX = 4095
LM, NWIN = 257, 3891
HOST_REPEATS = 3
N_SEQ = 4096


def model(rng):
    """(elog, erate, lam [K, D], logfact, mod_init, ltran): Gamma factors around per-column base rates."""
    import numpy as np
    from scipy.special import digamma, gammaln
    base = np.exp(rng.uniform(np.log(0.05), np.log(200.0), size=D))
    lam = base[None, :] * np.exp(0.3 * rng.normal(size=(K, D)))
    b = rng.uniform(0.5, 20.0, size=(K, D))
    a = lam * b
    vt = 1.0 + rng.random((K, K)) * 20 + 200 * np.eye(K)
    vi = rng.random(K) + 0.1
    return (digamma(a) - np.log(b), a / b, a / b, gammaln(np.arange(CMAX + 1.0) + 1.0),
            digamma(vi) - digamma(vi.sum()), digamma(vt) - digamma(vt.sum(1))[:, None])


def host_lliks(x, elog, erate, logfact):
    import numpy as np
    ok = ~np.isnan(x)
    c = np.where(ok, x, 0.0)
    ll = c.dot(elog.T) - ok.astype(np.float64).dot(erate.T)
    return ll - np.where(ok, logfact[c.astype(np.int64)], 0.0).sum(1)[:, None]


def host_stats(x, q):
    import numpy as np
    ok = ~np.isnan(x)
    return np.concatenate([q.T.dot(np.where(ok, x, 0.0)), q.T.dot(ok.astype(np.float64))], axis=1)


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
    elog, erate, lam, logfact, mod_init, ltran = model(rng)
    if case == "windows":
        T = NWIN * LM
        starts = np.arange(NWIN, dtype=np.int64) * LM
        lens = None
    else:
        lens = np.random.default_rng(20).integers(32, 513, size=N_SEQ).astype(np.int64)
        T = int(lens.sum())
    off = None if lens is None else np.concatenate(([0], np.cumsum(lens)))
    x = np.minimum(rng.poisson(lam[rng.integers(0, K, size=T)]), CMAX).astype(np.float64)
    x[rng.random((T, D)) < 0.02] = np.nan
    eng = HipEngine(0)
    eng.set_obs(x, None)
    eng.set_globals(mod_init, ltran)
    out = {}
    res = {"case": case, "route": route, "K": K, "D": D, "F": 2 * D, "rows": T}
    if route == "device":
        if lens is not None:
            eng.set_emission_poisson(elog, erate, CMAX)
            eng.set_sequences(lens)

        def call():
            eng.set_emission_poisson(elog, erate, CMAX)
            if lens is None:
                st = eng.estep(starts, LM, flags=L.TRANS_WRAP)
            else:
                st = eng.estep_sequences(flags=0)[0]
            out["counts"], out["lb"] = st.flat, float(st.lb[0])
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
            ll = host_lliks(x[a:a + n], elog, erate, logfact)
            eng.set_lliks(ll.reshape(len(st0), lm, K))
            st = eng.estep(st0, lm, flags=L.USE_HOST_LLIKS | (L.TRANS_WRAP if lens is None else 0))
            q = eng.read_intermediate("var_x", len(st0), lm).reshape(n, K)
            return host_stats(x[a:a + n], q), float(st.lb[0])

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
    ap.add_argument("--route", choices=["device", "host"])
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
        print("bench_poisson: no GPU (a time is only a time on the device)", file=sys.stderr)
        return 2
    results, rc = [], 0
    for case in ("windows", "sequences"):
        for route in ("device", "host"):
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
    doc = {"tool": "tools/bench_poisson.py", "device": device_name(), "summary": summary, "results": results}
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
