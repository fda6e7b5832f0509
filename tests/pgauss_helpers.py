"""NumPy statements of the Gaussian-tracks family (svihmm_set_emission_pgauss, include/svihmm.h): the llik loop of the
contract and the statistics [sxx | sx | n] about an origin, plus the data and models the tests share.  Host-side only."""
import numpy as np

MASK_AS_NAN = 1
ABSENT = 1e150
# Spread of the states' means around a column's base: mu_kd = base_d + sigma_d (SPREAD / sqrt(D)) N(0, 1).  The expected
# log-likelihood ratio of two states over a row is about sum_d delta_d^2 / 2 = O(SPREAD^2) whatever D is.
SPREAD = 3.0


def present(x):
    """ok bool[n, D]: entry (t, d) is present when x > -1e150 and x < 1e150 (a NaN fails both)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (x > -ABSENT) & (x < ABSENT)


def pgauss_lliks(x, mask, mu, hprec, cst, flags=0):
    """``ll[t, k] = s``: s starts at +0.0; per present column in ascending d, r = x - mu[k, d], p = r * r,
    p = p * hprec[k, d], s = s + p, s = s + cst[k, d], each a rounded operation of its own.  All +0.0 for a row masked
    under MASK_AS_NAN or without a present entry.  x [n, D], tables [K, D]."""
    x = np.asarray(x, dtype=np.float64)
    ok = present(x)
    if (flags & MASK_AS_NAN) and mask is not None:
        ok = ok & ~np.asarray(mask, dtype=bool)[:, None]
    s = np.zeros((x.shape[0], mu.shape[0]))
    for d in range(x.shape[1]):
        okd = ok[:, d]
        r = np.where(okd, x[:, d], 0.0)[:, None] - mu[:, d][None, :]
        p = r * r
        p = p * hprec[:, d][None, :]
        t = s + p
        t = t + cst[:, d][None, :]
        s = np.where(okd[:, None], t, s)
    return s


def pgauss_stats(x, mask, origin, q):
    """``[sxx | sx | n]`` [K, 3D] with r = x - origin[d]: sums of q[t, k] (r * r), q[t, k] r and q[t, k] over the rows
    with ``mask[t] == 0`` whose entry d is present.  Rows that contribute to no column are left out whatever q holds."""
    x = np.asarray(x, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    ok = present(x)
    if mask is not None:
        ok = ok & ~np.asarray(mask, dtype=bool)[:, None]
    live = ok.any(1)
    x, ok, q = x[live], ok[live], q[live]
    r = np.where(ok, np.where(ok, x, 0.0) - origin[None, :], 0.0)
    return np.concatenate([q.T.dot(r * r), q.T.dot(r), q.T.dot(ok.astype(np.float64))], axis=1)


def data_origin(x):
    """Each column's mean over its present entries (0 for a column without any)."""
    ok = present(x)
    cnt = ok.sum(0)
    return np.where(cnt > 0, np.where(ok, x, 0.0).sum(0) / np.maximum(cnt, 1), 0.0)


def residual_scale(x, mask, origin):
    """Largest |r| of the unmasked present entries (1 when there is none)."""
    ok = present(x) & ~np.asarray(mask, dtype=bool)[:, None]
    r = np.abs(np.where(ok, np.where(ok, x, 0.0) - origin[None, :], 0.0))
    return max(float(r.max()), 1.0)


def window_rows(starts, Lm):
    return (np.asarray(starts, dtype=np.int64)[:, None] + np.arange(Lm)[None, :]).ravel()


def tables(mu, nus, alphas, betas):
    from scipy.special import digamma
    return (np.ascontiguousarray(mu, dtype=np.float64), -0.5 * alphas / betas,
            -0.5 / nus - 0.5 * (np.log(betas) - digamma(alphas)) - 0.5 * np.log(2.0 * np.pi))


def make_model(K, D, rng):
    """A random model, through digamma as the classes form them: dict with mu / hprec / cst [K, D], means [K, D],
    sig [D] (the columns' spreads, log-uniform in [0.1, 10]), mod_init [K], ltran [K, K].  Column bases about 1e3."""
    from scipy.special import digamma
    base = 1e3 + rng.normal(size=D) * 20.0
    sig = np.exp(rng.uniform(np.log(0.1), np.log(10.0), size=D))
    means = base[None, :] + sig[None, :] * (SPREAD / np.sqrt(D)) * rng.normal(size=(K, D))
    nus = rng.uniform(1.0, 50.0, size=(K, D))
    alphas = rng.uniform(2.0, 20.0, size=(K, D))
    betas = alphas * (sig[None, :] * np.exp(0.2 * rng.normal(size=(K, D)))) ** 2
    mu, hprec, cst = tables(means, nus, alphas, betas)
    vt = 1.0 + rng.random((K, K)) * 20
    vi = rng.random(K) + 0.1
    return dict(mu=mu, hprec=hprec, cst=cst, means=means, sig=sig,
                mod_init=digamma(vi) - digamma(vi.sum()), ltran=digamma(vt) - digamma(vt.sum(1))[:, None])


def make_data(T, D, rng, means, sig, mask_frac=0.1):
    """[T, D] rows drawn from random states, with every kind of entry the contract names: about 10 % NaN entries, some
    +Inf / -Inf / 1e308 / -1e200, one column entirely absent (D > 1), rows without a present entry, masked rows."""
    z = rng.integers(0, means.shape[0], size=T)
    x = means[z] + sig[None, :] * rng.normal(size=(T, D))
    mask = rng.random(T) < mask_frac
    x[rng.random((T, D)) < 0.10] = np.nan
    for v in (np.inf, -np.inf, 1e308, -1e200):
        x[rng.random((T, D)) < 0.005] = v
    if D > 1:
        x[:, D // 2] = [(np.nan, np.inf, -1e200)[t % 3] for t in range(T)]      # a column without a present entry
    r = rng.permutation(T)[:6]
    x[r[0]] = np.nan
    x[r[1]] = [(np.nan, -np.inf, 1e308)[d % 3] for d in range(D)]               # every column absent
    x[r[2]] = np.inf
    x[r[3], 0] = -0.0
    mask[r[1:4]] = False
    mask[r[0]] = True
    return x, mask


# ---- the problems the CPU and the GPU tests share
T = 700
# (K, D): (3, 1) smallest; (16, 5) D no multiple of 4, tables in LDS, F = 15; (64, 21) F = 63, MT = 1; (65, 22) a second
# state group, strided lanes, F = 66, MT = 2; (17, 43) F = 129, MT = 4; (256, 33) K = 256, tables past 64 KB (read
# through L2); (64, 128) F = 384, two feature groups, the raised LDS limit
SHAPES = [(3, 1), (16, 5), (64, 21), (65, 22), (17, 43), (256, 33), (64, 128)]
IDS = ["K3D1", "K16D5", "K64D21", "K65D22", "K17D43", "K256D33", "K64D128"]
LENGTHS = (1, 2, 63, 64, 65, 257, 1)
_cache = {}


def problem(i):
    if i not in _cache:
        K, D = SHAPES[i]
        rng = np.random.default_rng(700 + i)
        p = make_model(K, D, rng)
        x, mask = make_data(T, D, rng, p["means"], p["sig"])
        p.update(K=K, D=D, x=x, mask=mask, origin=data_origin(x))
        _cache[i] = p
    return _cache[i]


def lliks_of(p, x=None, mask=None, flags=0):
    return pgauss_lliks(p["x"] if x is None else x, p["mask"] if mask is None else mask, p["mu"], p["hprec"],
                        p["cst"], flags)


def seq_problem(i):
    """The first sum(LENGTHS) rows of problem i as sequences of LENGTHS: (problem, offsets, rows)."""
    p = dict(problem(i))
    Ts = sum(LENGTHS)
    p["x"], p["mask"] = p["x"][:Ts], p["mask"][:Ts]
    off = np.zeros(len(LENGTHS) + 1, dtype=np.int64)
    np.cumsum(LENGTHS, out=off[1:])
    return p, off, Ts


def grow_case():
    """K = 16, five tracks from a sticky chain with 2 % of the entries missing; the states overlap, so the widths differ."""
    K, D = SHAPES[1]
    rng = np.random.default_rng(GROW_SEED)
    Tg = 600
    p = make_model(K, D, rng)
    sts = np.repeat(rng.integers(0, K, size=Tg // 25 + 1), 25)[:Tg]
    x = p["means"][sts] + p["sig"][None, :] * rng.normal(size=(Tg, D))
    x[rng.random((Tg, D)) < 0.02] = np.nan
    A = np.full((K, K), 0.1 / (K - 1))
    np.fill_diagonal(A, 0.9)
    p.update(K=K, D=D, x=x, mask=np.zeros(Tg, bool), origin=data_origin(x),
             mod_init=np.log(np.ones(K) / K), ltran=np.log(A))
    return p, Tg


GROW_SEED = 65      # (a seed whose compared residuals keep the factor-3 margin: asserted on the CPU, tests/test_pgauss_ref.py)
GROW_CENTERS = np.array([93, 116, 139, 162, 208, 231, 277, 300, 323, 346], dtype=np.int64)
GROW_RULE = dict(half0=4, m=0, inc=2, cutoff=60, eps=1e-5, rule=0)


def grow_compared(p, Tg):
    """Every residual the growth rule compares against epsilon, on the NumPy lliks."""
    from tests.grow_helpers import grow_direct
    ll = lliks_of(p)
    compared = []
    for c in GROW_CENTERS:
        grow_direct(ll, p["mod_init"], p["ltran"], Tg, int(c), compared=compared, **GROW_RULE)
    return np.array(compared), ll


# ---- held-out entries
def entry_terms(p, cols, vals):
    """``(term [n, K], ok [n], mag [n])``: t = x - mu, t = t * t, t = t * hprec, t = t + cst (each rounded on its own)
    for the present values; mag: the largest magnitude among the entry's operands and intermediates."""
    cols = np.asarray(cols, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.float64)
    ok = present(vals)
    x = np.where(ok, vals, 0.0)[:, None]
    mu, hp, cs = p["mu"][:, cols].T, p["hprec"][:, cols].T, p["cst"][:, cols].T
    t = x - mu
    t = t * t
    mag = np.maximum(np.abs(x[:, 0]), np.maximum(np.abs(mu).max(1), np.abs(t).max(1)))
    t = t * hp
    mag = np.maximum(mag, np.abs(t).max(1))
    t = t + cs
    mag = np.maximum(mag, np.maximum(np.abs(cs).max(1), np.abs(t).max(1)))
    return np.where(ok[:, None], t, 0.0), ok, np.where(ok, mag, 0.0)


def lse_rows(v):
    m = np.max(v, axis=1)
    return m + np.log(np.sum(np.exp(v - m[:, None]), axis=1))


def heldout_entries_numpy(p, q, rows, cols, vals):
    """``(lp [n], M [n])``: LSE_k(log(q[rows] + 1e-9) + term) per entry (NaN for absent values) and the magnitude M the
    bound is built from."""
    term, ok, mag = entry_terms(p, cols, vals)
    lq = np.log(q[np.asarray(rows, dtype=np.int64)] + 1e-9)
    return np.where(ok, lse_rows(lq + term), np.nan), np.maximum(mag, np.abs(lq).max(1))


def entry_list(p, n, seed):
    """n entries (rows, cols, vals) of which at least 90 % are present: values drawn around a random state's mean, about
    5 % of them NaN / Inf / sentinels."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, p["x"].shape[0], size=n)
    cols = rng.integers(0, p["D"], size=n)
    k = rng.integers(0, p["K"], size=n)
    vals = p["means"][k, cols] + p["sig"][cols] * rng.normal(size=n)
    bad = rng.random(n) < 0.05
    vals[bad] = rng.choice([np.nan, np.inf, -np.inf, 1e308, -1e200, 1e150, -1e150], size=int(bad.sum()))
    return rows.astype(np.int64), cols.astype(np.int32), vals
