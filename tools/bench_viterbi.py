"""Timing of svihmm_viterbi (Engine.viterbi) on one MI355X; bench.py is not involved.

    python tools/bench_viterbi.py [--out profiles/viterbi_bench.json] [--limit 300]

Every case runs in a child process of its own under a time limit (``--limit`` seconds); the first case
that fails, faults or runs out of time ends the run -- nothing else is started on the device after it.
Cases (BASELINE.json):
  k64_windows  configs[2] shape, K=64 D=32 T=1e6, decoded as the epoch's window batch (3891 x 257 rows)
  k64_chain    the same sequence as ONE chain (B=1, Lm=T): sequential forward pass on one wave,
               psi in HBM, chunked backtrack
  k64_host     NumPy Viterbi (tests/viterbi_helpers.py) on the first 1e5 rows of the device's own lliks,
               scaled to T, plus the lliks read-back a host decode needs; the device path of the same
               slice is checked against it (exact)
  k16          configs[1] shape, K=16 D=8 T=1e5: window batch and chain
Per case: wall time of the whole call (median of the repeats, the call ends in a stream
synchronisation), the kernel time of its two device phases from HIP events in a separate pass
(emission; max-plus sweep + backtrack), and the HBM floor of the decode itself: lliks read once plus
z (windows) or psi + path + z (chain) written, at the 4.4 TB/s the scaled sweeps' streams reach in
profiles/ and at the 8 TB/s of the data sheet."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

CASES = ["k64_windows", "k64_chain", "k64_host", "k16"]
BW_MEASURED, BW_SPEC = 4.4e12, 8.0e12
LDS_ROWS = 1008          # kernels_viterbi.h: vit_lds_rows(64)


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


def floor_ms(B, Lm, K):
    """Bytes the decode has to move (lliks in, result out), over the two bandwidths."""
    rows = B * Lm
    by = rows * K * 8 + rows * 4
    if Lm > LDS_ROWS:
        by += 3 * rows * 64          # psi written, read by the path kernel, path written (gather reads 1 of 64)
    return {"bytes": by, "ms_at_4.4TBs": by / BW_MEASURED * 1e3, "ms_at_8TBs": by / BW_SPEC * 1e3}


def timed(eng, starts, Lm, K, reps):
    import numpy as np
    starts = np.asarray(starts, dtype=np.int64)
    out = {}

    def call():
        out["z"], out["s"] = eng.viterbi(starts, Lm)
    med, lo, hi = median_ms(call, reps)
    eng.profile(True)
    eng.profile_reset()
    call()
    pr = eng.profile_read()
    eng.profile(False)
    rec = {"B": int(len(starts)), "Lm": int(Lm), "K": K, "call_ms": med, "call_ms_min": lo, "call_ms_max": hi,
           "repeats": reps, "emission_kernel_ms": pr.get("emission", (0.0, 0))[0],
           "viterbi_kernels_ms": pr.get("misc", (0.0, 0))[0], "d2h_ms": pr.get("d2h", (0.0, 0))[0],
           "floor": floor_ms(len(starts), Lm, K)}
    assert np.all(np.isfinite(out["s"])) and out["z"].min() >= 0 and out["z"].max() < K
    return rec, out["z"], out["s"]


def k64_problem(eng):
    import bench
    from _workload import bench_problem
    pb = bench_problem(eng)
    eng.set_globals(pb["mod_init"], pb["ltran"])
    eng.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
    return bench


def run_case(name):
    import numpy as np
    from pysvihmm_amd.engine import HipEngine
    eng = HipEngine(0)
    res = {"case": name}
    if name in ("k64_windows", "k64_chain", "k64_host"):
        bench = k64_problem(eng)
        K, T, LM = bench.K, bench.T, bench.LM
        if name == "k64_windows":
            st = np.arange(T // LM, dtype=np.int64) * LM
            res.update(timed(eng, st, LM, K, 20)[0])
        elif name == "k64_chain":
            res.update(timed(eng, [0], T, K, 5)[0])
        else:
            from tests.viterbi_helpers import viterbi_numpy
            n = 100000
            mi, lt = eng.read_globals()
            t0 = time.perf_counter()
            ll_all = eng.loglik([0], T)
            res["lliks_readback_ms"] = (time.perf_counter() - t0) * 1e3      # (includes the emission kernel, ~1 ms)
            res["lliks_bytes"] = int(ll_all.nbytes)
            ll = np.ascontiguousarray(ll_all[0, :n])
            del ll_all
            t0 = time.perf_counter()
            zr, sr = viterbi_numpy(ll, mi, lt)
            res["numpy_rows"] = n
            res["numpy_ms"] = (time.perf_counter() - t0) * 1e3
            res["numpy_ms_scaled_to_T"] = res["numpy_ms"] * T / n
            res["host_total_ms_scaled"] = res["numpy_ms_scaled_to_T"] + res["lliks_readback_ms"]
            rec, z, s = timed(eng, [0], n, K, 3)
            res["device_slice"] = rec
            res["device_equals_numpy"] = bool(np.array_equal(z[0], zr) and s[0] == sr)
            assert res["device_equals_numpy"]
    else:
        import bench
        from scipy.special import digamma  # noqa: F401
        K1, D1, T1, LM = 16, 8, 100000, bench.LM
        rs = np.random.RandomState(bench.SEED + 1)
        tran = 0.9 * np.eye(K1) + 0.1 / (K1 - 1) * (1.0 - np.eye(K1))
        means = rs.normal(0.0, 5.0, size=(K1, D1))
        chols = np.broadcast_to(np.eye(D1), (K1, D1, D1)).copy()
        eng.generate(tran, means, chols, T1, seed=bench.SEED + 1)
        obs = eng.read_generated(want_sts=False)[0]
        p1 = bench.variational_state(rs, means, obs[:20000], K1, D1, T1)
        eng.set_globals(p1["mod_init"], p1["ltran"])
        eng.set_emission_niw(p1["mu"], p1["sigma"], p1["kappa"], p1["nu"])
        st = np.arange(T1 // LM, dtype=np.int64) * LM
        res["windows"] = timed(eng, st, LM, K1, 20)[0]
        res["chain"] = timed(eng, [0], T1, K1, 10)[0]
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=300)
    args = ap.parse_args()
    if args.case:
        run_case(args.case)
        return 0
    if not os.path.exists("/dev/kfd"):
        print("bench_viterbi: no GPU (a time is only a time on the device)", file=sys.stderr)
        return 2
    results = []
    rc = 0
    for case in CASES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case], cwd=REPO,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.limit, text=True)
        except subprocess.TimeoutExpired:
            results.append({"case": case, "error": "time limit of %d s" % args.limit})
            rc = 1
            break
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            results.append({"case": case, "error": "exit status %d" % p.returncode, "stderr": p.stderr[-2000:]})
            rc = 1
            break          # nothing more on the device after a failure
        results.append(json.loads(line[-1][7:]))
        print(json.dumps(results[-1]), flush=True)
    doc = {"tool": "tools/bench_viterbi.py", "device": "MI355X", "results": results}
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
