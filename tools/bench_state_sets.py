"""Timing of the E-step under allowed-state sets (svihmm_set_state_sets) on one MI355X; bench.py is not involved.

    python tools/bench_state_sets.py [--out profiles/state_sets_bench.json] [--limit 900]

Epoch shape (tools/bench_labels.py's): K = 64 states, D = 32, T = 1e6 rows in 3891 windows of 257 rows, 10 % of the
rows constrained to a random set of 2 .. 8 states that holds the row's generating state.  Cases:
  niw        full-covariance NIW Gaussian emissions
  counts     32 Poisson count tracks
Routes, alternating in ONE process per case, one ``estep`` each, every call ending in a synchronise (the packed
statistics are read back):
  s  sets on the device: set_state_sets, then estep
  l  the same rows under single labels (each with its generating state): set_labels, then estep
  b  the host workaround: loglik read-back, NumPy clamp, set_lliks, estep(USE_HOST_LLIKS) -- all four timed
  c  the same handle with neither
Every route is warmed up once; then rounds of (s, l, c) -- and (b) while it still needs calls -- until each route has
at least 5 s of calls and at least 5 of them.  Reported: median and quartiles per route, s/l, s/b and s/c.  Sets and
labels are put on and taken off between the timed calls, outside them.  Separately (profiling on, after the timed
rounds): HIP-event time per kernel slot of routes s, l and c -- the emission slot's difference is the clamp kernel.
``--case X --route s|l|c --calls N`` runs N calls of one route and nothing else: the form a kernel trace is taken of.
Each case runs in a child process under a time limit; a child that fails ends the run."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.bench_labels import CMAX, D, FRAC, K, LM, MIN_CALLS, MIN_SECONDS, T, quartiles  # noqa: E402


def build(case):
    """(engine with rows, globals and family; packed sets uint64 [T, 1]; bool sets [T, K]; labels int32 [T])"""
    import numpy as np
    from scipy.special import digamma
    from pysvihmm_amd.engine import HipEngine
    from pysvihmm_amd.util import pack_state_sets
    rng = np.random.default_rng(11)
    sts = np.repeat(rng.integers(0, K, size=T // 50 + 1), 50)[:T]
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
        x = means[sts] + rng.normal(size=(T, D))
        eng.set_obs(x, None)
        eng.set_globals(mod_init, ltran)
        eng.set_emission_niw(means + 0.1 * rng.normal(size=(K, D)), np.tile((D + 2.0) * np.eye(D), (K, 1, 1)),
                             np.full(K, 1.0), np.full(K, D + 3.0))
    rows = np.flatnonzero(rng.random(T) < FRAC)
    lab = np.full(T, -1, dtype=np.int32)
    lab[rows] = sts[rows]
    allowed = np.ones((T, K), bool)
    size = rng.integers(2, 9, size=len(rows))                 # 2 .. 8 states: the generating one and random others
    score = rng.random((len(rows), K))
    score[np.arange(len(rows)), sts[rows]] = -1.0             # (the generating state ranks first)
    rank = np.argsort(np.argsort(score, axis=1), axis=1)
    allowed[rows] = rank < size[:, None]
    return eng, pack_state_sets(allowed), allowed, lab


def run_child(case, route, calls):
    import numpy as np
    from pysvihmm_amd import _lib as L
    eng, packed, allowed, lab = build(case)
    B = T // LM
    starts = np.arange(B, dtype=np.int64) * LM
    forbidden = ~allowed[:B * LM].reshape(B, LM, K)

    def estep(flags=0):
        return eng.estep(starts, LM, flags=L.TRANS_WRAP | flags)

    def route_b():
        ll = eng.loglik(starts, LM, 0)
        ll[forbidden] = -np.inf
        eng.set_lliks(ll)
        return estep(L.USE_HOST_LLIKS)

    def enter(n):
        if n == "s":
            eng.set_state_sets(packed, K=K)
        elif n == "l":
            eng.set_labels(lab)
        else:
            eng.set_state_sets(None)
            eng.set_labels(None)

    def timed(fn):
        t0 = time.perf_counter()
        st = fn()
        return (time.perf_counter() - t0) * 1e3, st

    if route:                                      # the form a kernel trace is taken of
        enter(route)
        for _ in range(calls + 1):
            estep()
        eng.close()
        print("RESULT " + json.dumps({"case": case, "route": route, "calls": calls}), flush=True)
        return
    names = ("s", "l", "b", "c")
    times = {n: [] for n in names}
    last = {}
    rnd = 0
    while True:
        need = [n for n in names if rnd == 0 or len(times[n]) < MIN_CALLS or sum(times[n]) < MIN_SECONDS * 1e3]
        if not need:
            break
        for n in names:
            if n not in need and n == "b":         # (the host route is far slower: only while it needs calls)
                continue
            enter(n)
            ms, st = timed(route_b if n == "b" else estep)
            last[n] = st.buf.copy()
            if rnd:                                # round 0 warms every route up
                times[n].append(ms)
        rnd += 1
    slots = {}
    for n in ("s", "l", "c"):
        enter(n)
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
    sizes = allowed.sum(axis=1)
    res = {"case": case, "K": K, "D": D, "rows": T, "constrained_rows": int(np.sum(sizes < K)),
           "mean_set_size": float(sizes[sizes < K].mean()), "windows": [int(B), LM],
           "routes": {n: quartiles(times[n]) for n in names}, "slot_ms": slots}
    med = {n: res["routes"][n]["median_ms"] for n in names}
    res["s_over_l"] = med["s"] / med["l"]
    res["s_over_b"] = med["s"] / med["b"]
    res["s_over_c"] = med["s"] / med["c"]
    res["clamp_ms"] = {n: slots[n].get("emission", 0.0) - slots["c"].get("emission", 0.0) for n in ("s", "l")}
    # the call under sets is defined as the host-lliks call on the clamped lliks
    res["s_vs_b_max_rel_diff"] = float(np.max(np.abs(last["s"] - last["b"]) / (1e-9 * T + np.abs(last["b"]))))
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["niw", "counts"])
    ap.add_argument("--route", choices=["s", "l", "c"], default=None)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=900)
    args = ap.parse_args()
    if args.case:
        run_child(args.case, args.route, args.calls)
        return 0
    if not os.path.exists("/dev/kfd"):
        print("bench_state_sets: no GPU (a time is only a time on the device)", file=sys.stderr)
        return 2
    env = dict(os.environ)
    for var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):       # at most 16 threads a child
        try:
            env[var] = str(max(1, min(int(env.get(var, "16")), 16)))
        except ValueError:
            env[var] = "16"
    results, rc = [], 0
    for case in ("niw", "counts"):
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
    doc = {"tool": "tools/bench_state_sets.py", "results": results}
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
