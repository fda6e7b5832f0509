"""Timing of svihmm_estep_sequences (Engine.estep_sequences) on one MI355X; bench.py is not involved.

    python tools/bench_sequences.py [--out profiles/sequences_bench.json] [--parent-lib build_ab_parent/libsvihmm_hip.so]
                                    [--limit 600] [--rounds 2]

Cases (K = 64, D = 32, the bench's generated process and variational state):
  a  4096 sequences, lengths drawn uniformly from [32, 512] (about 1.1e6 rows)
  b  the single-device form of BASELINE.json configs[3]: 8 sequences of 1e6 rows
  c  one sequence of 2047 rows alone (just below the whole-chain threshold): the forward_backward slot of the
     profile over 2046 steps is the ragged wave kernel's time per step of ONE wavefront
Routes:
  new   one estep_sequences call (statistics read back, the call ends in a stream synchronisation)
  loop  one estep([off], len, flags=0) per sequence, each read back, the sum formed on the host -- the only route
        before svihmm_estep_sequences existed.  With --parent-lib it runs on that library (a build of the parent
        commit, loaded through SVIHMM_HIP_LIB) as well as on the current one.
Every (case, route, library) runs in a child process of its own under a time limit; the libraries alternate
(--rounds passes over the list) so that neither always runs on a warmer device.  The first child that fails,
faults or runs out of time ends the run -- nothing else is started on the device after it.  Per child: median
wall time of the repeats after two warm-up calls, and in a separate pass the kernel time per profile slot from
HIP events."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

NEW_SYMBOLS = ("svihmm_set_sequences", "svihmm_estep_sequences")


def lengths_of(case):
    import numpy as np
    if case == "a":
        return np.random.default_rng(20).integers(32, 513, size=4096).astype(np.int64)
    if case == "b":
        return np.full(8, 1000000, dtype=np.int64)
    return np.array([2047], dtype=np.int64)


def median_ms(fn, n, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def run_child(case, route):
    import numpy as np
    from pysvihmm_amd import _lib as L
    if route == "loop" and "SVIHMM_HIP_LIB" in os.environ:
        for n in NEW_SYMBOLS:              # (a build of the parent commit does not export them)
            L.SIGNATURES.pop(n, None)
    import bench
    from pysvihmm_amd.engine import HipEngine
    lens = lengths_of(case)
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    T = int(off[-1])
    eng = HipEngine(0)
    rs, tran, means, chols = bench.true_process(0)
    eng.generate(tran, means, chols, T, seed=bench.SEED)
    head = eng.read_generated(want_sts=False)[0][:20000] if T <= 2000000 else None
    if head is None:                       # (8e6 x 32 doubles: read the head through a second, short sequence)
        e2 = HipEngine(0)
        e2.generate(tran, means, chols, 20000, seed=bench.SEED)
        head = e2.read_generated(want_sts=False)[0]
        e2.close()
    pb = bench.variational_state(rs, means, head)
    eng.set_globals(pb["mod_init"], pb["ltran"])
    eng.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
    out = {}
    if route == "new":
        eng.set_sequences(lens)

        def call():
            st, seq_lb, q0 = eng.estep_sequences(flags=0)
            out["buf"], out["lb"] = st.buf, seq_lb
    else:
        def call():
            tot, lbs = None, np.empty(len(lens))
            for s in range(len(lens)):
                st = eng.estep([int(off[s])], int(lens[s]), flags=0)
                lbs[s] = st.lb[0]
                tot = st.buf.copy() if tot is None else tot + st.buf
            out["buf"], out["lb"] = tot, lbs
    reps = {"a": 5, "b": 5, "c": 20}[case]
    med, lo, hi = median_ms(call, reps)
    eng.profile(True)
    eng.profile_reset()
    call()
    pr = eng.profile_read()
    eng.profile(False)
    assert np.all(np.isfinite(out["buf"]))
    res = {"case": case, "route": route, "lib": os.environ.get("SVIHMM_HIP_LIB", "current"), "N": int(len(lens)),
           "rows": T, "call_ms": med, "call_ms_min": lo, "call_ms_max": hi, "repeats": reps,
           "kernel_ms": {k: round(v[0], 4) for k, v in pr.items() if v[1]},
           "launches": {k: int(v[1]) for k, v in pr.items() if v[1]},
           "lb_total": float(np.sum(out["lb"])), "neff_total": float(out["buf"][64 * 64 + 64 * 32:64 * 64 + 64 * 32 + 64].sum())}
    if case == "c" and route == "new":
        res["ragged_us_per_step"] = pr["forward_backward"][0] * 1e3 / (int(lens[0]) - 1)
    if case == "a" and route == "new":
        # both directions of 4096 sequences in one launch: the launch over the steps of its longest sequence,
        # and over all steps of all units (throughput)
        fb = pr["forward_backward"][0]
        res["ragged_launch_us_per_longest_step"] = fb * 1e3 / (int(lens.max()) - 1)
        res["ragged_ns_per_unit_step"] = fb * 1e6 / (2.0 * float((lens - 1).sum()))
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["a", "b", "c"])
    ap.add_argument("--route", choices=["new", "loop"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="library built from the parent commit (path relative to the repository)")
    ap.add_argument("--limit", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--cases", default="c,a,b")
    args = ap.parse_args()
    if args.case:
        run_child(args.case, args.route)
        return 0
    if not os.path.exists("/dev/kfd"):
        print("bench_sequences: no GPU (a time is only a time on the device)", file=sys.stderr)
        return 2
    plan = []
    for rnd in range(args.rounds):
        for case in args.cases.split(","):
            if case != "c" and args.parent_lib:
                plan.append((rnd, case, "loop", args.parent_lib))
            plan.append((rnd, case, "new", None))
            if case != "c":
                plan.append((rnd, case, "loop", None))
    results, rc = [], 0
    for rnd, case, route, lib in plan:
        env = dict(os.environ)
        env.pop("SVIHMM_HIP_LIB", None)
        if lib:
            env["SVIHMM_HIP_LIB"] = os.path.join(REPO, lib)
        tag = {"round": rnd, "case": case, "route": route, "lib": lib or "current"}
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--route", route], cwd=REPO,
                               env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.limit, text=True)
        except subprocess.TimeoutExpired:
            results.append(dict(tag, error="time limit of %d s" % args.limit))
            rc = 1
            break
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            results.append(dict(tag, error="exit status %d" % p.returncode, stderr=p.stderr[-2000:]))
            rc = 1
            break          # nothing more on the device after a failure
        results.append(dict(json.loads(line[-1][7:]), **tag))
        print(json.dumps(results[-1]), flush=True)
    # ratios: loop on the parent's library (else on the current one) over the new call, best round of each
    summary = {}
    for case in ("a", "b"):
        best = {}
        for r in results:
            if r.get("case") == case and "call_ms" in r:
                key = (r["route"], "parent" if r["lib"] != "current" else "current")
                best[key] = min(best.get(key, float("inf")), r["call_ms"])
        if ("new", "current") in best:
            s = {"new_ms": best[("new", "current")]}
            for which in ("parent", "current"):
                if ("loop", which) in best:
                    s["loop_%s_ms" % which] = best[("loop", which)]
                    s["loop_%s_over_new" % which] = best[("loop", which)] / best[("new", "current")]
            summary[case] = s
    doc = {"tool": "tools/bench_sequences.py", "device": "MI355X", "summary": summary, "results": results}
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
