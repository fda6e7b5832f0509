"""Timing of svihmm_estep_sequence_subset (Engine.estep_sequence_subset) on one MI355X; bench.py is not involved.

    python tools/bench_seq_minibatch.py [--out profiles/seq_minibatch_bench.json]
                                        [--parent-lib build_ab_parent/libsvihmm_hip.so] [--limit 300] [--rounds 1]

Case (K = 64, D = 32, the bench's generated process and variational state): N = 4096 sequences, lengths drawn
uniformly from [32, 512] (about 1.1e6 rows), resident on the device.  A minibatch is M of them, one fixed seeded
draw without replacement, sorted ascending; M in {64, 256, 1024, 4096}.
Routes:
  subset    one estep_sequence_subset(idx) call on the current library
  full      one estep_sequences call over all N -- what hmmbatchsgd pays per iteration without minibatches.  On the
            current library (against subset at M = 4096: the difference is the gather) and, with --parent-lib, on a
            build of the parent commit loaded through SVIHMM_HIP_LIB
  reupload  the only way to the subset's statistics without the call: set_obs of the compacted rows + set_sequences +
            estep_sequences per iteration, the upload included (the rows are compacted on the host once, outside the
            timed region).  On the parent's library with --parent-lib, else on the current one
Every (route, M, library) runs in a child process of its own under a time limit.  The first child that fails, faults
or runs out of time ends the run -- nothing else is started on the device after it.  Per child: two warm-up calls,
the median wall time of 5 calls (each ends in a stream synchronisation with the statistics read back), and in a
separate pass the kernel time per profile slot from HIP events; subset's "misc" slot is the gather launch."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

NEW_SYMBOLS = ("svihmm_estep_sequence_subset",)
SIZES = (64, 256, 1024, 4096)
N_SEQ = 4096


def lengths():
    import numpy as np
    return np.random.default_rng(20).integers(32, 513, size=N_SEQ).astype(np.int64)


def draw(M):
    import numpy as np
    return np.sort(np.random.default_rng(1000 + M).choice(N_SEQ, size=M, replace=False)).astype(np.int32)


def median_ms(fn, n=5, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def run_child(route, M):
    import numpy as np
    from pysvihmm_amd import _lib as L
    if "SVIHMM_HIP_LIB" in os.environ:
        for n in NEW_SYMBOLS:              # (a build of the parent commit does not export them)
            L.SIGNATURES.pop(n, None)
    import bench
    from pysvihmm_amd.engine import HipEngine
    lens = lengths()
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    T = int(off[-1])
    idx = draw(M)
    R = int(lens[idx].sum())
    eng = HipEngine(0)
    rs, tran, means, chols = bench.true_process(0)
    eng.generate(tran, means, chols, T, seed=bench.SEED)
    obs = eng.read_generated(want_sts=False)[0]
    pb = bench.variational_state(rs, means, obs[:20000])
    eng.set_globals(pb["mod_init"], pb["ltran"])
    eng.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
    out = {}
    if route == "subset":
        eng.set_sequences(lens)

        def call():
            st, seq_lb, q0 = eng.estep_sequence_subset(idx, flags=0)
            out["buf"], out["lb"] = st.buf, seq_lb
    elif route == "full":
        eng.set_sequences(lens)

        def call():
            st, seq_lb, q0 = eng.estep_sequences(flags=0)
            out["buf"], out["lb"] = st.buf, seq_lb
    else:
        rows = np.ascontiguousarray(np.concatenate([obs[off[s]:off[s + 1]] for s in idx], axis=0))
        sub_lens = lens[idx]

        def call():
            eng.set_obs(rows, None)
            eng.set_sequences(sub_lens)
            st, seq_lb, q0 = eng.estep_sequences(flags=0)
            out["buf"], out["lb"] = st.buf, seq_lb
    med, lo, hi = median_ms(call)
    eng.profile(True)
    eng.profile_reset()
    call()
    pr = eng.profile_read()
    eng.profile(False)
    assert np.all(np.isfinite(out["buf"]))
    res = {"route": route, "M": int(M), "lib": os.environ.get("SVIHMM_HIP_LIB", "current"), "N": N_SEQ, "rows_total": T,
           "rows_listed": R if route != "full" else T, "call_ms": med, "call_ms_min": lo, "call_ms_max": hi, "repeats": 5,
           "kernel_ms": {k: round(v[0], 4) for k, v in pr.items() if v[1]},
           "launches": {k: int(v[1]) for k, v in pr.items() if v[1]},
           "lb_total": float(np.sum(out["lb"])),
           "neff_total": float(out["buf"][64 * 64 + 64 * 32:64 * 64 + 64 * 32 + 64].sum())}
    if route == "subset":
        g = pr.get("misc", (0.0, 0))
        res["gather_ms"] = g[0]
        res["gather_launches"] = int(g[1])
        res["gather_gb_per_s"] = (2.0 * R * 32 * 8 / 1e9) / (g[0] * 1e-3) if g[0] > 0 else None
        res["gather_share_of_kernel_time"] = g[0] / max(sum(v[0] for k, v in pr.items() if k not in ("h2d", "d2h")), 1e-9)
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=["subset", "full", "reupload"])
    ap.add_argument("--M", type=int, default=N_SEQ)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="library built from the parent commit (path relative to the repository)")
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=1)
    args = ap.parse_args()
    if args.route:
        run_child(args.route, args.M)
        return 0
    if not os.path.exists("/dev/kfd"):
        print("bench_seq_minibatch: no GPU (a time is only a time on the device)", file=sys.stderr)
        return 2
    plan = []
    for rnd in range(args.rounds):
        for M in SIZES:
            plan.append((rnd, "subset", M, None))
            plan.append((rnd, "reupload", M, args.parent_lib))
        plan.append((rnd, "full", N_SEQ, None))
        if args.parent_lib:
            plan.append((rnd, "full", N_SEQ, args.parent_lib))
    results, rc = [], 0
    for rnd, route, M, lib in plan:
        env = dict(os.environ)
        env.pop("SVIHMM_HIP_LIB", None)
        if lib:
            env["SVIHMM_HIP_LIB"] = os.path.join(REPO, lib)
        tag = {"round": rnd, "route": route, "M": M, "lib": lib or "current"}
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--route", route, "--M", str(M)], cwd=REPO,
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
    # per M: the new call against both routes that exist without it, best round of each
    best = {}
    for r in results:
        if "call_ms" in r:
            key = (r["route"], r["M"], "parent" if r["lib"] != "current" else "current")
            best[key] = min(best.get(key, float("inf")), r["call_ms"])
    which = "parent" if args.parent_lib else "current"
    summary = {"reupload_and_full_lib": which}
    full_other = best.get(("full", N_SEQ, which))
    for M in SIZES:
        if ("subset", M, "current") not in best:
            continue
        s = {"subset_ms": best[("subset", M, "current")]}
        if ("reupload", M, which) in best:
            s["reupload_ms"] = best[("reupload", M, which)]
            s["reupload_over_subset"] = s["reupload_ms"] / s["subset_ms"]
        if full_other is not None:
            s["full_ms"] = full_other
            s["full_over_subset"] = full_other / s["subset_ms"]
        g = [r for r in results if r.get("route") == "subset" and r.get("M") == M and "gather_ms" in r]
        if g:
            s["gather_ms"] = g[-1]["gather_ms"]
            s["gather_share_of_kernel_time"] = g[-1]["gather_share_of_kernel_time"]
        summary["M=%d" % M] = s
    if ("subset", N_SEQ, "current") in best and ("full", N_SEQ, "current") in best:
        summary["all_listed_minus_full_current_ms"] = best[("subset", N_SEQ, "current")] - best[("full", N_SEQ, "current")]
        summary["full_current_ms"] = best[("full", N_SEQ, "current")]
    doc = {"tool": "tools/bench_seq_minibatch.py", "device": "MI355X", "summary": summary, "results": results}
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
