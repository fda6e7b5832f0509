"""Per-iteration cost of ``hmmbatchsgd.VBHMM(seq_minibatch=M).infer()`` on one MI355X: the resident SVI loop on
sequence minibatches (``device_loop=True``) against the host route (``device_loop=False``: the same kernels plus
SciPy psi, the emission upload, the statistics read-back, the NumPy natural-gradient step and ``lower_bound()`` per
iteration -- the behaviour before the loop existed).  bench.py is not involved.

    python tools/bench_svi_sequences.py [--out profiles/svi_sequences_bench.json] [--iters 100] [--warmup 20]
                                        [--rounds 2] [--families niw,mcat,poisson] [--sizes 64,256]

Case: K = 64; N = 4096 sequences, lengths drawn uniformly from [32, 512] (about 1.1e6 rows); M = 64 and 256;
  niw      NIW Gaussian emitters, D = 32
  mcat     ProductCategorical, 32 binary tracks
  poisson  ProductPoisson, 32 count tracks
Both routes alternate in ONE process on one model definition (device, host, device, host, ..: ``--rounds`` of each),
every run from the same seed and the same initial factors, ``maxit = warmup + iters``.
What is timed, per run, over the ``iters`` iterations behind the warm-up:
  host route    wall time from the start of one iteration to the start of the next (its E-step call, the step, and
                ``lower_bound()``): median and mean
  device loop   the calls only enqueue, so a per-iteration wall clock would time the enqueue: the loop's wall time is
                taken from the first timed ``svi_iteration_sequences`` call to the return of ``svi_read_elbo`` (which
                waits for the device) divided by the iterations -- a mean that holds the whole tail; beside it the
                median of the host's enqueue intervals and the median device time per iteration from
                ``svi_read_elbo``
The upload, ``svi_begin*`` and the final E-step over all sequences are outside both.  The best round of each route is
compared; ``ratio`` = host median / device-loop wall."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

K, D, N_SEQ, MAXC = 64, 32, 4096, 60


def lengths():
    import numpy as np
    return np.random.default_rng(20).integers(32, 513, size=N_SEQ).astype(np.int64)


def data(fam):
    """list of N_SEQ arrays [T_s, D] from a sticky K-state chain"""
    import numpy as np
    lens = lengths()
    T = int(lens.sum())
    rng = np.random.default_rng({"niw": 1, "mcat": 2, "poisson": 3}[fam])
    sts = np.repeat(rng.integers(0, K, size=T // 16 + 1), 16)[:T]
    if fam == "niw":
        obs = (3.0 * rng.normal(size=(K, D)))[sts] + rng.normal(size=(T, D))
    elif fam == "mcat":
        p1 = rng.beta(0.5, 0.5, size=(K, D))
        obs = (rng.random((T, D)) < p1[sts]).astype(np.float64)
    else:
        rate = rng.uniform(0.5, 20.0, size=(K, D))
        obs = np.minimum(rng.poisson(rate[sts]), MAXC).astype(np.float64)
    off = np.concatenate(([0], np.cumsum(lens)))
    return [obs[off[s]:off[s + 1]] for s in range(N_SEQ)], obs


def model(fam, seqs, rows, M, maxit, engine):
    import numpy as np
    from pysvihmm_amd import hmmbatchsgd
    from pysvihmm_amd.distributions import Gaussian, ProductCategorical, ProductPoisson
    np.random.seed(5)
    if fam == "niw":
        mu0, sg0 = rows[:50000].mean(0), 0.75 * np.cov(rows[:50000].T)
        emit = np.array([Gaussian(mu_0=mu0, sigma_0=sg0, kappa_0=0.01, nu_0=D + 2) for _ in range(K)])
    elif fam == "mcat":
        emit = np.array([ProductCategorical(alphav_0=[np.ones(2) * 1.5] * D) for _ in range(K)])
    else:
        emit = np.array([ProductPoisson(np.full(D, 2.0), np.full(D, 0.5), max_count=MAXC) for _ in range(K)])
    return hmmbatchsgd.VBHMM(seqs, np.ones(K), np.ones((K, K)), emit, maxit=maxit, seq_minibatch=M, engine=engine)


def run(fam, seqs, rows, M, device_loop, warmup, iters, engine):
    """one infer(); -> dict of the figures over the `iters` iterations behind the warm-up"""
    import numpy as np
    m = model(fam, seqs, rows, M, warmup + iters, engine)
    stamps, done = [], {}
    if device_loop:
        assert m._svi_sequences_refusal() is None, m._svi_sequences_refusal()
        it_call, read = engine.svi_iteration_sequences, engine.svi_read_elbo

        def iteration(*a, **kw):
            stamps.append(time.perf_counter())
            return it_call(*a, **kw)

        def read_elbo(n):
            out = read(n)
            done["t"] = time.perf_counter()
            done["ms"] = np.array(out[1])
            return out

        engine.svi_iteration_sequences, engine.svi_read_elbo = iteration, read_elbo
    else:
        stats = m._seq_minibatch_stats

        def minibatch():
            stamps.append(time.perf_counter())
            return stats()

        m._seq_minibatch_stats = minibatch
    np.random.seed(77)
    try:
        m.infer(device_loop=device_loop)
        t_end = time.perf_counter()
    finally:
        if device_loop:
            del engine.svi_iteration_sequences, engine.svi_read_elbo
    assert len(stamps) == warmup + iters and np.all(np.isfinite(m.elbo_vec)) and len(m.elbo_vec) == warmup + iters
    gaps = np.diff(np.array(stamps[warmup:])) * 1e3
    res = {"family": fam, "M": M, "route": "device_loop" if device_loop else "host", "iterations": iters, "warmup": warmup,
           "elbo_last": float(m.elbo_vec[-1])}
    if device_loop:
        res["wall_ms"] = (done["t"] - stamps[warmup]) * 1e3 / iters
        res["enqueue_ms_median"] = float(np.median(gaps))
        res["device_ms_median"] = float(np.median(done["ms"][warmup:]))
        res["device_ms_mean"] = float(np.mean(done["ms"][warmup:]))
        res["recoveries"] = engine.svi_recoveries()
    else:
        res["wall_ms"] = float(np.median(gaps))
        res["wall_ms_mean"] = float(np.mean(gaps))
        res["estep_and_step_ms_median"] = float(np.median(m.iter_time[warmup:]) * 1e3)
    res["infer_s"] = t_end - stamps[0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--families", default="niw,mcat,poisson")
    ap.add_argument("--sizes", default="64,256")
    args = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        print("bench_svi_sequences: no GPU (a time is only a time on the device)", file=sys.stderr)
        return 2
    from pysvihmm_amd.engine import HipEngine
    results, summary = [], {}
    for fam in args.families.split(","):
        seqs, rows = data(fam)
        engine = HipEngine(0)
        try:
            for M in (int(s) for s in args.sizes.split(",")):
                best = {}
                for rnd in range(args.rounds):
                    for dl in (True, False):
                        r = run(fam, seqs, rows, M, dl, args.warmup, args.iters, engine)
                        r["round"] = rnd
                        results.append(r)
                        print(json.dumps(r), flush=True)
                        best[r["route"]] = min(best.get(r["route"], float("inf")), r["wall_ms"])
                dev = [r for r in results if r["family"] == fam and r["M"] == M and r["route"] == "device_loop"]
                summary["%s M=%d" % (fam, M)] = {
                    "host_ms_per_iteration": best["host"], "device_loop_ms_per_iteration": best["device_loop"],
                    "ratio": best["host"] / best["device_loop"],
                    "device_ms_median": min(r["device_ms_median"] for r in dev)}
        finally:
            engine.close()
    doc = {"tool": "tools/bench_svi_sequences.py", "device": "MI355X", "K": K, "D": D, "N": N_SEQ,
           "rows_total": int(lengths().sum()), "summary": summary, "results": results}
    print(json.dumps({"summary": summary}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
