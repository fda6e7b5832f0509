"""NumPy statements of the Poisson count family (svihmm_set_emission_poisson, include/svihmm.h): the llik loop
of the contract and the statistics [sx | n], plus the data and models the tests share.  Host-side only."""
import numpy as np

MASK_AS_NAN = 1
# Spread of the states' rates around a column's base rate: lambda_kd = base_d exp(s N(0, 1)) with
# s = SPREAD / sqrt(sum_d base_d).  The expected log-likelihood ratio of two states over a row is about
# sum_d lambda_d delta_d^2 / 2 = O(SPREAD^2) whatever D and the rates are, so one value serves every shape.
# Tuned on the CPU: at 1.5 every row of every data set is soft, at 8 fewer than 4 % of the (16, 128) rows are; at 4 the
# share of rows with max_k q < 0.99 is between 0.27 (K = 3) and 1.0 (K = 64).
# The GPU test asserts on the referee's posteriors that at least a tenth of each data set's rows have max_k q < 0.99,
# so that the statistics tests compare more than one-hot rows.
SPREAD = 4.0


def logfact_table(C):
    from scipy.special import gammaln
    return gammaln(np.arange(C + 1, dtype=np.float64) + 1.0)


def present(x, C):
    """``(c int[n, D], ok bool[n, D])``: entry (t, d) is present when x >= 0.0 and x < (double)(C + 1) (a NaN fails
    both); its count is (int)x."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = (x >= 0.0) & (x < float(C + 1))
    return np.where(ok, x, 0.0).astype(np.int64), ok


def poisson_lliks(x, mask, elog, erate, logfact, flags=0):
    """``ll[t, k] = s - g``: s and g start at +0.0; per present column in ascending d, p = c * elog[k, d] (a rounded
    multiply of its own), s = s + p, s = s - erate[k, d], g = g + logfact[c].  All +0.0 for a row masked under
    MASK_AS_NAN or without a present entry.  x [n, D], elog / erate [K, D]."""
    x = np.asarray(x, dtype=np.float64)
    elog = np.asarray(elog, dtype=np.float64)
    erate = np.asarray(erate, dtype=np.float64)
    logfact = np.asarray(logfact, dtype=np.float64)
    c, ok = present(x, len(logfact) - 1)
    if (flags & MASK_AS_NAN) and mask is not None:
        ok = ok & ~np.asarray(mask, dtype=bool)[:, None]
    s = np.zeros((x.shape[0], elog.shape[0]))
    g = np.zeros(x.shape[0])
    for d in range(x.shape[1]):
        okd = ok[:, d]
        p = c[:, d].astype(np.float64)[:, None] * elog[:, d][None, :]
        s = np.where(okd[:, None], s + p, s)
        s = np.where(okd[:, None], s - erate[:, d][None, :], s)
        g = np.where(okd, g + logfact[c[:, d]], g)
    return s - g[:, None]


def poisson_stats(x, mask, C, q):
    """``[sx | n]`` [K, 2D]: sx[k, d] = sum q[t, k] c_td, n[k, d] = sum q[t, k], over rows with ``mask[t] == 0``
    whose entry d is present.  Rows that contribute to no column are left out whatever q holds there."""
    x = np.asarray(x, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    c, ok = present(x, C)
    if mask is not None:
        ok = ok & ~np.asarray(mask, dtype=bool)[:, None]
    live = ok.any(1)
    c, ok, q = c[live], ok[live], q[live]
    sx = q.T.dot(np.where(ok, c, 0).astype(np.float64))
    n = q.T.dot(ok.astype(np.float64))
    return np.concatenate([sx, n], axis=1)


def window_rows(starts, Lm):
    return (np.asarray(starts, dtype=np.int64)[:, None] + np.arange(Lm)[None, :]).ravel()


def make_model(K, D, rng, base=None):
    """A random model, through digamma as the classes form them: dict with elog / erate [K, D], lam [K, D] (the
    means a / b), mod_init [K], ltran [K, K].  Base rates per column log-uniform in [0.05, 200] (``base``: given
    ones), lambda_kd = base_d exp(s N(0, 1)), b in [0.5, 20], a = lambda b."""
    from scipy.special import digamma
    if base is None:
        base = np.exp(rng.uniform(np.log(0.05), np.log(200.0), size=D))
    base = np.asarray(base, dtype=np.float64)
    s = SPREAD / np.sqrt(base.sum())
    lam = base[None, :] * np.exp(s * rng.normal(size=(K, D)))
    b = rng.uniform(0.5, 20.0, size=(K, D))
    a = lam * b
    vt = 1.0 + rng.random((K, K)) * 20
    ltran = digamma(vt) - digamma(vt.sum(1))[:, None]
    vi = rng.random(K) + 0.1
    return dict(elog=digamma(a) - np.log(b), erate=a / b, lam=a / b, base=base,
                mod_init=digamma(vi) - digamma(vi.sum()), ltran=ltran)


def make_data(T, D, C, rng, lam=None, mask_frac=0.1):
    """Count matrix [T, D] (rows drawn from random states of ``lam`` [K, D]; rate 5 without it) with every kind of
    entry the contract names: single NaN entries, whole NaN rows, a row whose every column is absent (mixed NaN, -1 and
    C + 1), masked rows, one entry equal to C (present) and one equal to C + 1 (absent) on unmasked rows, a +inf, a
    -0.5 and a 3.7."""
    if lam is None:
        lam = np.full((1, D), 5.0)
    z = rng.integers(0, lam.shape[0], size=T)
    x = np.minimum(rng.poisson(lam[z]), C).astype(np.float64)
    mask = rng.random(T) < mask_frac
    if T >= 16:
        x[rng.random((T, D)) < 0.05] = np.nan
        x[rng.random(T) < 0.04] = np.nan
        r = rng.permutation(T)[:8]
        x[r[0]] = np.nan
        x[r[1]] = [(-1.0, np.nan, float(C + 1))[d % 3] for d in range(D)]      # every column absent
        x[r[2], D - 1] = float(C)                                     # the last count the table holds
        x[r[3], 0] = float(C + 1)                                     # one past it
        x[r[4], D - 1] = np.inf
        x[r[5], 0] = -0.5
        x[r[6], D - 1] = 3.7
        mask[r[1:7]] = False
        mask[r[0]] = True
    return x, mask


# ---- the problems the CPU and the GPU tests share
T = 700
C = 4095
# K = 3 and 16: ragged state tiles, F = 4 and 14 below one feature tile; K = 65: a second state group of one state;
# (256, 40): F = 80, more than one 64-feature group, tables beyond 64 KB (read through L2); (16, 128): D at the limit
SHAPES = [(3, 2), (16, 7), (64, 12), (65, 3), (256, 40), (16, 128)]
IDS = ["K3", "K16", "K64", "K65", "K256", "D128"]
LENGTHS = (1, 2, 63, 64, 65, 257, 1)
FFBS_SEED = 0       # for every shape the NumPy paths of this seed have no step near a CDF boundary (asserted on the CPU)
FFBS_DRAWS = 3
_cache = {}


def problem(i):
    if i not in _cache:
        K, D = SHAPES[i]
        rng = np.random.default_rng(200 + i)
        base = np.exp(rng.uniform(np.log(0.05), np.log(200.0), size=D))
        if i == 2:
            base[5] = 3000.0            # counts reach the table's upper range
        p = make_model(K, D, rng, base)
        x, mask = make_data(T, D, C, rng, lam=p["lam"])
        p.update(K=K, D=D, C=C, x=x, mask=mask, logfact=logfact_table(C))
        _cache[i] = p
    return _cache[i]


def lliks_of(p, x=None, mask=None, flags=0):
    return poisson_lliks(p["x"] if x is None else x, p["mask"] if mask is None else mask, p["elog"], p["erate"],
                         p["logfact"], flags)


def seq_problem(i):
    """The first sum(LENGTHS) rows of problem i as sequences of LENGTHS: (problem, offsets, rows)."""
    p = dict(problem(i))
    Ts = sum(LENGTHS)
    p["x"], p["mask"] = p["x"][:Ts], p["mask"][:Ts]
    off = np.zeros(len(LENGTHS) + 1, dtype=np.int64)
    np.cumsum(LENGTHS, out=off[1:])
    return p, off, Ts


def ffbs_reference(i):
    """(la_ref [Ts, K], u [S, Ts], z_np [S, Ts], off) of the FFBS test: the C referee's forward filter per sequence
    on the NumPy lliks and the NumPy backward draws of FFBS_SEED's uniforms."""
    from oracle import ref_c
    from tests.decode_sequences_helpers import backward_sample_sequences
    p, off, Ts = seq_problem(i)
    ll = lliks_of(p)
    la = np.concatenate([ref_c.forward(np.ascontiguousarray(ll[int(a):int(b)]), p["mod_init"], p["ltran"])
                         for a, b in zip(off[:-1], off[1:])])
    u = np.random.default_rng(FFBS_SEED).random((FFBS_DRAWS, Ts))
    return la, u, backward_sample_sequences(la, p["ltran"], u, off), off


def grow_case():
    """K = 16, seven count tracks from a sticky chain; the states overlap, so the widths differ."""
    K, D = SHAPES[1]
    rng = np.random.default_rng(32)          # (a seed whose compared residuals keep the factor-3 margin, see the tests)
    Tg = 600
    p = make_model(K, D, rng, base=np.array([0.3, 1.0, 2.0, 4.0, 8.0, 20.0, 60.0]))
    sts = np.repeat(rng.integers(0, K, size=Tg // 25 + 1), 25)[:Tg]
    x = rng.poisson(p["lam"][sts]).astype(np.float64)
    A = np.full((K, K), 0.1 / (K - 1))
    np.fill_diagonal(A, 0.9)
    p.update(K=K, D=D, C=C, x=x, mask=np.zeros(Tg, bool), logfact=logfact_table(C),
             mod_init=np.log(np.ones(K) / K), ltran=np.log(A))
    return p, Tg


GROW_CENTERS = np.array([93, 116, 139, 162, 208, 231, 277, 300, 323, 346], dtype=np.int64)
GROW_RULE = dict(half0=4, m=0, inc=2, cutoff=60, eps=1e-5, rule=0)
