"""Timing of svihmm_viterbi_sequences / svihmm_ffbs_sequences (Engine.viterbi_sequences / .ffbs_sequences) on one
MI355X; bench.py is not involved.

    python tools/bench_decode_sequences.py [--out profiles/decode_sequences_bench.json]
                                           [--parent-lib build_exp/libsvihmm_parent.so] [--limit 600] [--rounds 1]

Cases (the generator and variational state of tools/bench_sequences.py: K = 64, D = 32, 4096 sequences with lengths
drawn uniformly from [32, 512], about 1.1e6 rows):
  vit     MAP paths of all sequences
  ffbs1   one FFBS draw of every sequence (device uniforms)
  ffbs16  sixteen draws of every sequence from one filter
  wide    MAP paths at K = 100: 512 sequences with lengths from [100, 600] -- every sequence above 240 rows keeps psi
          in HBM and is backtracked through the common chunk run
Routes:
  new    one call for all sequences (results read back, the call ends in a stream synchronisation)
  loop   one viterbi([off], len) / ffbs_windows([off], len, ..) call per sequence -- the only route before the two
         calls existed.  With --parent-lib it runs on that library (a build of the parent commit, loaded through
         SVIHMM_HIP_LIB) as well as on the current one.
Every (case, route, library) runs in a child process of its own under a time limit; the first child that fails,
faults or runs out of time ends the run -- nothing else is started on the device after it.  Per child: median wall
time of 5 calls after two warm-up calls, and in a separate pass the kernel time per profile slot from HIP events."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_sequences import median_ms  # noqa: E402

NEW_SYMBOLS = ("svihmm_viterbi_sequences", "svihmm_ffbs_sequences")
CASES = ("vit", "ffbs1", "ffbs16", "wide")


def lengths_of(case):
    import numpy as np
    if case == "wide":
        return np.random.default_rng(21).integers(100, 601, size=512).astype(np.int64)
    return np.random.default_rng(20).integers(32, 513, size=4096).astype(np.int64)


def wide_state(head, K, seed):
    """A K-state variational state on the generated rows: factors centred on K of the rows themselves."""
    import numpy as np
    from scipy.special import digamma
    rng = np.random.default_rng(seed)
    D = head.shape[1]
    var_tran = 1.0 + rng.random((K, K)) * 4.0 + 40.0 * np.eye(K)
    vi = 1.0 + rng.random(K)
    return {"mod_init": digamma(vi) - digamma(vi.sum()),
            "ltran": digamma(var_tran) - digamma(var_tran.sum(1)[:, None]),
            "mu": head[rng.choice(head.shape[0], size=K, replace=False)].copy(),
            "sigma": np.broadcast_to(np.cov(head.T) * (D + 4.0), (K, D, D)).copy(),
            "kappa": np.full(K, 5.0), "nu": np.full(K, D + 4.0)}


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
    head = eng.read_generated(want_sts=False)[0][:20000]
    pb = wide_state(head, 100, 5) if case == "wide" else bench.variational_state(rs, means, head)
    eng.set_globals(pb["mod_init"], pb["ltran"])
    eng.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
    logA = np.ascontiguousarray(pb["ltran"])
    S = {"ffbs1": 1, "ffbs16": 16}.get(case, 0)
    out = {}
    if route != "loop":
        eng.set_sequences(lens)
        if S:
            def call():
                out["z"] = eng.ffbs_sequences(logA, n_draws=S, seed=7)[0]
        else:
            def call():
                out["z"], out["score"] = eng.viterbi_sequences()
    elif S:
        def call():
            z = np.empty((S, T), dtype=np.int32)
            for s in range(len(lens)):
                a, n = int(off[s]), int(lens[s])
                z[:, a:a + n] = eng.ffbs_windows([a], n, logA, n_draws=S, seed=7)[0][:, 0]
            out["z"] = z
    else:
        def call():
            z, score = np.empty(T, dtype=np.int32), np.empty(len(lens))
            for s in range(len(lens)):
                a, n = int(off[s]), int(lens[s])
                zz, sc = eng.viterbi([a], n)
                z[a:a + n], score[s] = zz[0], sc[0]
            out["z"], out["score"] = z, score
    med, lo, hi = median_ms(call, 5)
    eng.profile(True)
    eng.profile_reset()
    call()
    pr = eng.profile_read()
    eng.profile(False)
    assert out["z"].min() >= 0 and out["z"].max() < eng.K
    res = {"case": case, "route": route, "lib": os.environ.get("SVIHMM_HIP_LIB", "current"), "K": int(eng.K),
           "N": int(len(lens)), "rows": T, "draws": S, "call_ms": med, "call_ms_min": lo, "call_ms_max": hi, "repeats": 5,
           "kernel_ms": {k: round(v[0], 4) for k, v in pr.items() if v[1]},
           "launches": {k: int(v[1]) for k, v in pr.items() if v[1]},
           "z_checksum": int(out["z"].astype(np.int64).sum())}
    if "score" in out:
        res["score_total"] = float(np.sum(out["score"]))
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--route", choices=["new", "loop"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="library built from the parent commit (path relative to the repository)")
    ap.add_argument("--limit", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--cases", default=",".join(CASES))
    args = ap.parse_args()
    if args.case:
        run_child(args.case, args.route)
        return 0
    if not os.path.exists("/dev/kfd"):
        print("bench_decode_sequences: no GPU (a time is only a time on the device)", file=sys.stderr)
        return 2
    plan = []
    for rnd in range(args.rounds):
        for case in args.cases.split(","):
            if args.parent_lib:
                plan.append((rnd, case, "loop", args.parent_lib))
            plan.append((rnd, case, "new", None))
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
    for case in CASES:
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
    doc = {"tool": "tools/bench_decode_sequences.py", "device": "MI355X", "summary": summary, "results": results}
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
