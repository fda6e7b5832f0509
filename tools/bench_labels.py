"""Timing of the E-step on partially labelled rows (svihmm_set_labels) on one MI355X; bench.py is not involved.

    python tools/bench_labels.py [--out profiles/labels_bench.json] [--limit 900]

Epoch shape: K = 64 states, D = 32, T = 1e6 rows in 3891 windows of 257 rows, 10 % of the rows labelled (each with its
generating state).  Cases:
  niw        full-covariance NIW Gaussian emissions
  counts     32 Poisson count tracks
  sequences  NIW, 4096 sequences of 32 .. 512 rows (about 1.1e6 rows) through estep_sequences: labelled against
             unlabelled only (that call takes no host lliks, so there is no host route to compare with)
Routes of the window cases, alternating in ONE process per case, one ``estep`` each, every call ending in a
synchronise (the packed statistics are read back):
  a  labelled on the device: set_labels, then estep
  b  the host workaround: loglik read-back, NumPy clamp, set_lliks, estep(USE_HOST_LLIKS) -- all four timed
  c  the same handle with the labels removed
Every route is warmed up once; then rounds of (a, c) -- and (b) while it still needs calls -- until each route has at
least 5 s of calls and at least 5 of them.  Reported: median and quartiles per route, a/b and a/c.  The labels are put
on and taken off between the timed calls, outside them.  Separately (profiling on, after the timed rounds): HIP-event
time per kernel slot of routes a and c.
``--case X --route a|c --calls N`` runs N calls of one route and nothing else: the form a kernel trace is taken of.
Each case runs in a child process under a time limit; a child that fails ends the run."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

K, D, T, LM = 64, 32, 1000000, 257
CMAX = 4095
FRAC = 0.10
N_SEQ = 4096
MIN_SECONDS, MIN_CALLS = 5.0, 5


def quartiles(ts):
    import numpy as np
    q = np.percentile(np.asarray(ts), [25, 50, 75])
    return {"median_ms": float(q[1]), "q1_ms": float(q[0]), "q3_ms": float(q[2]), "calls": len(ts),
            "seconds": float(np.sum(ts)) * 1e-3}


def build(case):
    """(engine with rows, globals and family; labels int32 [T]; lengths or None)"""
    import numpy as np
    from scipy.special import digamma
    from pysvihmm_amd.engine import HipEngine
    rng = np.random.default_rng(11)
    lens = None
    rows = T
    if case == "sequences":
        lens = np.random.default_rng(20).integers(32, 513, size=N_SEQ).astype(np.int64)
        rows = int(lens.sum())
    sts = np.repeat(rng.integers(0, K, size=rows // 50 + 1), 50)[:rows]
    vt = 1.0 + rng.random((K, K)) * 20 + 200 * np.eye(K)
    vi = rng.random(K) + 0.1
    mod_init, ltran = digamma(vi) - digamma(vi.sum()), digamma(vt) - digamma(vt.sum(1))[:, None]
    eng = HipEngine(0)
    if case == "counts":
        base = np.exp(rng.uniform(np.log(0.05), np.log(200.0), size=D))
        lam = base[None, :] * np.exp(0.3 * rng.normal(size=(K, D)))
        b = rng.uniform(0.5, 20.0, size=(K, D))
        a = lam * b
        x = np.minimum(rng.poisson(lam[sts]), CMAX).astype(np.float64)
        eng.set_obs(x, None)
        eng.set_globals(mod_init, ltran)
        eng.set_emission_poisson(digamma(a) - np.log(b), a / b, CMAX)
    else:
        means = rng.normal(0.0, 5.0, size=(K, D))
        x = means[sts] + rng.normal(size=(rows, D))
        eng.set_obs(x, None)
        eng.set_globals(mod_init, ltran)
        eng.set_emission_niw(means + 0.1 * rng.normal(size=(K, D)), np.tile((D + 2.0) * np.eye(D), (K, 1, 1)),
                             np.full(K, 1.0), np.full(K, D + 3.0))
    if lens is not None:
        eng.set_sequences(lens)
    lab = np.where(rng.random(rows) < FRAC, sts, -1).astype(np.int32)
    return eng, lab, lens


def run_child(case, route, calls):
    import numpy as np
    from pysvihmm_amd import _lib as L
    eng, lab, lens = build(case)
    B = T // LM
    starts = np.arange(B, dtype=np.int64) * LM
    lw = None if lens is not None else lab[:B * LM].reshape(B, LM)
    lrows = None if lw is None else np.nonzero(lw >= 0)

    def estep(flags=0):
        if lens is None:
            return eng.estep(starts, LM, flags=L.TRANS_WRAP | flags)
        return eng.estep_sequences(flags=flags)[0]

    def route_b():
        ll = eng.loglik(starts, LM, 0)
        keep = ll[lrows[0], lrows[1], lw[lrows]]
        ll[lrows[0], lrows[1], :] = -np.inf
        ll[lrows[0], lrows[1], lw[lrows]] = keep
        eng.set_lliks(ll)
        return estep(L.USE_HOST_LLIKS)

    def timed(fn):
        t0 = time.perf_counter()
        st = fn()
        return (time.perf_counter() - t0) * 1e3, st

    if route:                                      # the form a kernel trace is taken of
        eng.set_labels(lab if route == "a" else None)
        for _ in range(calls + 1):
            estep()
        eng.close()
        print("RESULT " + json.dumps({"case": case, "route": route, "calls": calls}), flush=True)
        return
    names = ("a", "c") if lens is not None else ("a", "b", "c")
    times = {n: [] for n in names}
    last = {}
    rnd = 0
    while True:
        need = [n for n in names if rnd == 0 or len(times[n]) < MIN_CALLS or sum(times[n]) < MIN_SECONDS * 1e3]
        if not need:
            break
        for n in names:
            if n not in need and n == "b":         # (the host route is three orders slower: only while it needs calls)
                continue
            eng.set_labels(lab if n == "a" else None)
            ms, st = timed(route_b if n == "b" else estep)
            last[n] = st.buf.copy()
            if rnd:                                # round 0 warms every route up
                times[n].append(ms)
        rnd += 1
    # per-slot kernel time of routes a and c: HIP events around the launches, a pass of its own
    slots = {}
    for n in ("a", "c"):
        eng.set_labels(lab if n == "a" else None)
        estep()
        eng.profile(True)
        acc = {}
        for _ in range(10):
            eng.profile_reset()
            estep()
            for k, (ms, cnt) in eng.profile_read().items():
                acc.setdefault(k, []).append(ms)
        eng.profile(False)
        slots[n] = {k: float(np.median(v)) for k, v in acc.items()}
    res = {"case": case, "K": K, "D": D, "rows": int(len(lab)), "labelled_rows": int(np.sum(lab >= 0)),
           "windows": None if lens is not None else [int(B), LM], "sequences": None if lens is None else int(len(lens)),
           "routes": {n: quartiles(times[n]) for n in names}, "slot_ms": slots}
    med = {n: res["routes"][n]["median_ms"] for n in names}
    res["a_over_c"] = med["a"] / med["c"]
    if "b" in med:
        res["a_over_b"] = med["a"] / med["b"]
        # the labelled call is defined as the host-lliks call on the clamped lliks
        res["a_vs_b_max_rel_diff"] = float(np.max(np.abs(last["a"] - last["b"]) / (1e-9 * len(lab) + np.abs(last["b"]))))
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["niw", "counts", "sequences"])
    ap.add_argument("--route", choices=["a", "c"], default=None)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=900)
    args = ap.parse_args()
    if args.case:
        run_child(args.case, args.route, args.calls)
        return 0
    if not os.path.exists("/dev/kfd"):
        print("bench_labels: no GPU (a time is only a time on the device)", file=sys.stderr)
        return 2
    env = dict(os.environ)
    for var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):       # at most 16 threads a child
        try:
            env[var] = str(max(1, min(int(env.get(var, "16")), 16)))
        except ValueError:
            env[var] = "16"
    results, rc = [], 0
    for case in ("niw", "counts", "sequences"):
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
    doc = {"tool": "tools/bench_labels.py", "results": results}
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
