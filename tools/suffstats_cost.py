"""Cost of the statistics step of the host loops, host against device (svihmm_suffstats), K = 64, D = 32.

  metaobs : hmmsgd_metaobs.VBHMM subclass overriding forward_msgs (so infer() runs its host loop):
            S = 64 windows of Lm = 257 per minibatch.  host = intermediate_pars per window, accumulated
            as the loop does (reference hmmsgd_metaobs.py:857-904); route = the loop's _segments_inter
            (stacking the windows' posteriors, idempotent uploads, one suffstats call, conversion).
  batch   : hmmbatchcd.VBHMM subclass overriding local_update, the whole chain at T = 1e5 and 1e6.
            host = the literal global_update (hmmbatchcd.py:172-189: np.outer per row + K weighted
            meanfieldupdate passes); route = _batch_suffstats + _global_update_from_stats.
            The host figure at T = 1e6 is extrapolated linearly from T = 1e5 unless --host-1e6.
Device kernel times (statistics GEMM + finalize, host-to-device copy) come from the engine's profile slots.
Prints one JSON object per scenario.   python tools/suffstats_cost.py [--reps N] [--host-1e6]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pysvihmm_amd import hmmbatchcd, hmmsgd_metaobs, util  # noqa: E402
from pysvihmm_amd.distributions import Gaussian  # noqa: E402
from pysvihmm_amd.engine import HipEngine  # noqa: E402

K, D = 64, 32


class MsgMeta(hmmsgd_metaobs.VBHMM):
    def forward_msgs(self, metaobs=None):
        super(MsgMeta, self).forward_msgs(metaobs)


class LocalBatch(hmmbatchcd.VBHMM):
    def local_update(self, obs=None, mask=None):
        super(LocalBatch, self).local_update(obs, mask)


def _emit(rng, obs):
    m0, c0 = obs.mean(0), np.cov(obs[:20000].T)
    return np.array([Gaussian(mu=m0 + rng.normal(size=D), sigma=c0.copy(), mu_0=m0, sigma_0=0.75 * c0,
                              kappa_0=0.01, nu_0=D + 2.0) for _ in range(K)])


def _obs(rng, T):
    means = rng.normal(0, 3, size=(K, D))
    sts = np.repeat(rng.integers(0, K, size=T // 50 + 1), 50)[:T]
    return means[sts] + rng.normal(size=(T, D)), rng.random(T) < 0.05


def _posteriors(rng, shape):
    q = rng.random(shape)
    return q / q.sum(-1, keepdims=True)


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def _kernels(eng, fn, reps):
    eng.profile(True)
    eng.profile_reset()
    for _ in range(reps):
        fn()
    eng.sync()
    p = eng.profile_read()
    eng.profile(False)
    return {k: p[k][0] / reps for k in ("stats", "finalize", "h2d") if k in p}


def metaobs(eng, reps, S=64, L=128):
    rng = np.random.default_rng(1)
    T = 200000
    obs, mask = _obs(rng, T)
    m = MsgMeta(obs, np.ones(K), np.ones((K, K)) + 1.0, _emit(rng, obs), metaobs_half=L, mb_sz=S, mask=mask,
                maxit=1, seed=1, engine=eng)
    m._psi_expectations()
    m._upload_obs()
    m._push_globals()
    m._push_emission()
    Lm = 2 * L + 1
    starts = rng.integers(0, T - Lm, size=S)
    q = _posteriors(rng, (S, Lm, K))
    segs = [(int(s), int(s) + Lm - 1, q[b]) for b, s in enumerate(starts)]

    def host():
        A = np.zeros((K, K))
        E = [util.NIW_zero_nat_pars(m.var_emit[0]) for _ in range(K)]
        for b, s in enumerate(starts):
            A_i, e_i = m._intermediate(q[b], int(s), int(s) + Lm - 1)
            A += A_i
            for k in range(K):
                E[k] += e_i[k]
        return A, E

    def route():
        return m._segments_inter(segs, None, None)

    A_h, E_h = host()
    A_r, E_r = route()
    dev = np.abs(A_r - A_h).max() / np.abs(A_h).max()
    t_host = _median_ms(host, max(1, reps // 10))
    t_route = _median_ms(route, reps)
    t_call = _median_ms(lambda: eng.suffstats(starts, Lm, q), reps)
    kern = _kernels(eng, lambda: eng.suffstats(starts, Lm, q), reps)
    return dict(scenario="metaobs", K=K, D=D, S=S, Lm=Lm, host_ms=t_host, route_ms=t_route,
                suffstats_call_ms=t_call, device_ms=kern, upload_MB=q.nbytes / 2 ** 20,
                A_rel_diff=float(dev), speedup=t_host / t_route)


def batch(eng, reps, T, host_full):
    rng = np.random.default_rng(T)
    obs, mask = _obs(rng, T)
    m = LocalBatch(obs, np.ones(K), np.ones((K, K)), _emit(rng, obs), mask=mask, maxit=1, engine=eng)
    m.var_x = _posteriors(rng, (T, K))
    m.mod_init, m.mod_tran = np.zeros(K), np.zeros((K, K))

    def route():
        m._global_update_from_stats(m._batch_suffstats())

    t_route = _median_ms(route, reps)
    q = m.var_x[None]
    t_call = _median_ms(lambda: eng.suffstats([0], T, q, flags=0), reps)
    kern = _kernels(eng, lambda: eng.suffstats([0], T, q, flags=0), reps)
    vt_route = m.var_tran.copy()
    out = dict(scenario="batch", K=K, D=D, T=T, route_ms=t_route, suffstats_call_ms=t_call, device_ms=kern,
               upload_MB=q.nbytes / 2 ** 20)
    if host_full:
        t0 = time.perf_counter()
        hmmbatchcd.VBHMM.global_update(m)
        out["host_ms"] = (time.perf_counter() - t0) * 1e3
        out["var_tran_rel_diff"] = float(np.abs(m.var_tran - vt_route).max() / np.abs(vt_route).max())
        out["speedup"] = out["host_ms"] / t_route
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-1e6", action="store_true", help="time the host global_update at T = 1e6 too (minutes)")
    a = ap.parse_args()
    eng = HipEngine(0)
    print(json.dumps(metaobs(eng, a.reps)), flush=True)
    r5 = batch(eng, a.reps, 100000, True)
    print(json.dumps(r5), flush=True)
    r6 = batch(eng, max(3, a.reps // 4), 1000000, a.host_1e6)
    if "host_ms" not in r6:
        r6["host_ms_extrapolated"] = r5["host_ms"] * 10
        r6["speedup"] = r6["host_ms_extrapolated"] / r6["route_ms"]
    print(json.dumps(r6), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
