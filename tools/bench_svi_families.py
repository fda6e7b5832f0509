"""Timing of the resident SVI loop on the multi-column Categorical and Poisson families (svihmm_svi_begin_mcat /
svihmm_svi_begin_poisson) on one MI355X; bench.py is not involved.

    python tools/bench_svi_families.py [--out profiles/svi_families_bench.json] [--limit 420]
    python tools/bench_svi_families.py --workload mcat|poisson     # device iterations only (for a kernel trace)

Model: K = 64 states, 32 binary tracks (F = 64), respectively 32 count tracks (counts up to 4095), T = 1e6 rows.
A minibatch is 64 windows of 257 rows (metaobs_half = 128).
Routes, per family:
  device     svihmm_svi_iteration: per iteration the window starts and three scalars go to the device.  Device time per
             iteration from svihmm_svi_read_elbo's stamps, wall time per iteration from the block's submission to the
             ELBO read-back.
  host       the only route that existed at engine level before the loop took these families: SciPy tables ->
             set_globals + set_emission_* -> estep (statistics read back) -> the NumPy rules and the ELBO terms.
             Wall time per iteration.
  class      hmmsgd_metaobs.VBHMM.infer: wall time per iteration of the whole call after the observations are
             resident (svi_begin .. state read-back), and the median of its iter_time.
device and host alternate in one process, in blocks of BLOCK iterations, after one warm-up block each; every route
gets at least 200 timed iterations.  Each family runs in a child process of its own under a time limit and with at
most 16 threads; the first child that fails ends the run -- nothing else is started on the device after it."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

K, D, T = 64, 32, 1000000
HALF, NWIN = 128, 64
LM = 2 * HALF + 1
CMAX = 4095
BLOCK, NBLOCKS = 50, 4


def problem(fam, rng):
    """(obs [T, D], prior blocks, factor blocks, prior_tran, var_tran)"""
    import numpy as np
    sts = np.repeat(rng.integers(0, K, size=T // 50 + 1), 50)[:T]
    if fam == "mcat":
        p1 = rng.beta(0.5, 0.5, size=(K, D))
        obs = (rng.random((T, D)) < p1[sts]).astype(np.float64)
        prior = [np.full((K, 2), 1.5) for _ in range(D)]
        fac = [1.0 + 5.0 * rng.random((K, 2)) for _ in range(D)]
    else:
        lam = np.exp(rng.uniform(np.log(0.05), np.log(200.0), size=D))[None, :] * np.exp(0.3 * rng.normal(size=(K, D)))
        obs = np.minimum(rng.poisson(lam[sts]), CMAX).astype(np.float64)
        prior = [np.full((K, D), 2.0), np.full((K, D), 0.5)]
        fac = [4.0 * lam * np.exp(0.2 * rng.normal(size=(K, D))), np.full((K, D), 4.0)]
    return obs, prior, fac, np.ones((K, K)), 1.0 + 10.0 * rng.random((K, K)) + 100.0 * np.eye(K)


def begin(eng, fam, pt, vt, prior, fac, maxit):
    if fam == "mcat":
        eng.svi_begin_mcat(pt, vt, prior, fac, maxit)
    else:
        eng.svi_begin_poisson(pt, vt, prior, fac, CMAX, maxit)


def host_iteration(eng, fam, pt, vt, prior, fac, starts, rho, bA, bE):
    """One iteration of the host-stepped route -> (var_tran, factors, elbo)"""
    import numpy as np
    from scipy.special import digamma, gammaln
    from pysvihmm_amd import _lib as L
    from pysvihmm_amd.hmmbase import dirichlet_elbo
    A_mean = vt / vt.sum(1)[:, None]
    pi = np.linalg.solve(A_mean.T - np.eye(K) + 1.0, np.ones(K))
    vi = pi / np.sqrt(pi @ pi)
    eng.set_globals(digamma(vi + 1e-9) - digamma(vi.sum() + 1e-9), digamma(vt + 1e-9) - digamma(vt.sum(1)[:, None] + 1e-9))
    if fam == "mcat":
        eng.set_emission_mcat([digamma(a) - digamma(a.sum(1))[:, None] for a in fac])
    else:
        eng.set_emission_poisson(digamma(fac[0]) - np.log(fac[1]), fac[0] / fac[1], CMAX)
    st = eng.estep(starts, LM, flags=L.TRANS_WRAP)
    n = len(starts)
    vt = ((1.0 - rho) * (vt - 1.0) + rho * (bA * (st.A_raw + n * (pt - 1.0)))) + 1.0
    if fam == "mcat":
        fac = [((1.0 - rho) * (a - 1.0) + (rho * bE) * (n * (a0 - 1.0) + c)) + 1.0 for a, a0, c in zip(fac, prior, st.col_counts)]
        vlb = 0.0
        for a, a0 in zip(fac, prior):
            el = digamma(a) - digamma(a.sum(1))[:, None]
            vlb += float(np.sum(gammaln(a0.sum(1)) - gammaln(a.sum(1))) + np.sum((a0 - a) * el - gammaln(a0) + gammaln(a)))
    else:
        a0, b0 = prior
        a, b = (1.0 - rho) * fac[0] + rho * (a0 + bE * st.sx), (1.0 - rho) * fac[1] + rho * (b0 + bE * st.n)
        fac = [a, b]
        vlb = -float(np.sum((a - a0) * digamma(a) - gammaln(a) + gammaln(a0) + a0 * (np.log(b) - np.log(b0)) + a * (b0 - b) / b))
    return vt, fac, float(st.lb[0]) + dirichlet_elbo(pt, vt) + vlb


def stats_of(ts):
    ts = sorted(ts)
    return {"median": ts[len(ts) // 2], "q1": ts[len(ts) // 4], "q3": ts[3 * len(ts) // 4], "min": ts[0], "max": ts[-1],
            "n": len(ts)}


def run_child(fam, workload=False):
    import numpy as np
    from pysvihmm_amd import _lib as L
    from pysvihmm_amd import hmmsgd_metaobs
    from pysvihmm_amd.distributions import ProductCategorical, ProductPoisson
    from pysvihmm_amd.engine import HipEngine
    rng = np.random.default_rng(11)
    obs, prior, fac0, pt, vt0 = problem(fam, rng)
    bA = (T - 2 * HALF - 1) / (2.0 * HALF * NWIN)
    bE = (T - 2 * HALF - 1) / ((2.0 * HALF + 1.0) * NWIN)
    eng = HipEngine(0)
    eng.set_obs(obs, None)
    draw = lambda: rng.integers(0, T - LM, size=NWIN).astype(np.int64)
    flags = L.TRANS_WRAP | L.KEEP_LBETA

    def device_block(n):
        """n iterations from the initial state -> (device ms per iteration [n], wall ms per iteration, elbo [n])"""
        begin(eng, fam, pt, vt0, prior, fac0, n)
        eng.sync()
        t0 = time.perf_counter()
        for it in range(n):
            eng.svi_iteration(it, draw(), NWIN, LM, flags, (it + 1.0) ** -0.7, bA, bE)
        e, ms = eng.svi_read_elbo(n)
        wall = (time.perf_counter() - t0) * 1e3 / n
        assert eng.svi_recoveries() == 0 and np.all(np.isfinite(e))
        return list(ms), wall, e

    if workload:
        ms, wall, _ = device_block(300)
        print("RESULT " + json.dumps({"family": fam, "device_ms_median": sorted(ms)[150], "wall_ms": wall}), flush=True)
        eng.close()
        return

    def host_block(n):
        vt, fac, ts, e = vt0.copy(), [f.copy() for f in fac0], [], []
        for it in range(n):
            st = draw()
            t0 = time.perf_counter()
            vt, fac, el = host_iteration(eng, fam, pt, vt, prior, fac, st, (it + 1.0) ** -0.7, bA, bE)
            ts.append((time.perf_counter() - t0) * 1e3)
            e.append(el)
        assert np.all(np.isfinite(e))
        return ts

    device_block(BLOCK); host_block(BLOCK // 5)                # warm-up
    dev_ms, dev_wall, host_ms = [], [], []
    for _ in range(NBLOCKS):
        ms, wall, _ = device_block(BLOCK)
        dev_ms += ms[1:]            # (the first iteration of a block starts behind svi_begin's uploads)
        dev_wall.append(wall)
        host_ms += host_block(BLOCK)
    # the class: wall time of infer() per iteration once the observations are resident
    np.random.seed(3)
    if fam == "mcat":
        emit = np.array([ProductCategorical(alphav_0=[np.full(2, 1.5)] * D) for _ in range(K)])
    else:
        emit = np.array([ProductPoisson(np.full(D, 2.0), np.full(D, 0.5), max_count=CMAX) for _ in range(K)])
    maxit = BLOCK * NBLOCKS
    m = hmmsgd_metaobs.VBHMM(obs, np.ones(K), np.ones((K, K)), emit, metaobs_half=HALF, mb_sz=NWIN, maxit=maxit, seed=3,
                             engine=eng)
    assert m._svi_device_ok()
    m.infer()
    w = m.infer_wall_ms
    cls_wall = (w["svi_begin"] + w["submit_iterations"] + w["wait_and_read_state"] + w["last_window"]) / maxit
    assert np.all(np.isfinite(m.elbo_vec)) and eng.svi_recoveries() == 0
    res = {"family": fam, "K": K, "D": D, "T": T, "windows": NWIN, "Lm": LM,
           "device_ms_per_iteration": stats_of(dev_ms), "device_wall_ms_per_iteration": stats_of(dev_wall),
           "host_stepped_wall_ms_per_iteration": stats_of(host_ms),
           "class_infer_wall_ms_per_iteration": cls_wall, "class_infer_upload_obs_ms": w["upload_obs"],
           "class_iter_time_ms_median": float(np.median(m.iter_time[1:]) * 1e3), "class_iterations": maxit}
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", choices=["mcat", "poisson"])
    ap.add_argument("--workload", choices=["mcat", "poisson"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=420)
    args = ap.parse_args()
    if args.workload:
        run_child(args.workload, workload=True)
        return 0
    if args.family:
        run_child(args.family)
        return 0
    if not os.path.exists("/dev/kfd"):
        print("bench_svi_families: no GPU (a time is only a time on the device)", file=sys.stderr)
        return 2
    from tools.bench_poisson import device_name
    env = dict(os.environ)
    for var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):       # at most 16 threads a child
        try:
            env[var] = str(max(1, min(int(env.get(var, "16")), 16)))
        except ValueError:
            env[var] = "16"
    results, rc = [], 0
    for fam in ("mcat", "poisson"):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--family", fam], cwd=REPO,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.limit, text=True, env=env)
        except subprocess.TimeoutExpired:
            results.append({"family": fam, "error": "time limit of %d s" % args.limit})
            rc = 1
            break
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            results.append({"family": fam, "error": "exit status %d" % p.returncode, "stderr": p.stderr[-2000:]})
            rc = 1
            break              # nothing more on the device after a failure
        results.append(json.loads(line[-1][7:]))
        print(json.dumps(results[-1]), flush=True)
    summary = {r["family"]: {"device_ms": r["device_ms_per_iteration"]["median"],
                             "device_wall_ms": r["device_wall_ms_per_iteration"]["median"],
                             "host_stepped_wall_ms": r["host_stepped_wall_ms_per_iteration"]["median"],
                             "class_infer_wall_ms": r["class_infer_wall_ms_per_iteration"],
                             "host_stepped_over_device_wall": r["host_stepped_wall_ms_per_iteration"]["median"]
                             / r["device_wall_ms_per_iteration"]["median"]}
               for r in results if "error" not in r}
    doc = {"tool": "tools/bench_svi_families.py", "device": device_name(), "summary": summary, "results": results}
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
