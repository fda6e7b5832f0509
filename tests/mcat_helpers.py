"""NumPy statements of the multi-column Categorical family (svihmm_set_emission_mcat, include/svihmm.h):
the llik loop of the contract and the symbol counts, plus the data the tests share.  Host-side only."""
import numpy as np

MASK_AS_NAN = 1


def offsets_of(V):
    off = np.zeros(len(V) + 1, dtype=np.int64)
    np.cumsum(np.asarray(V, dtype=np.int64), out=off[1:])
    return off


def present(x, V):
    """``(xi int[n, D], ok bool[n, D])``: entry (t, d) is present when it is not NaN and 0 <= (int)x < V[d]."""
    x = np.asarray(x, dtype=np.float64)
    nan = np.isnan(x)
    xi = np.trunc(np.where(nan, -1.0, x)).astype(np.int64)
    ok = (~nan) & (xi >= 0) & (xi < np.asarray(V, dtype=np.int64)[None, :])
    return np.where(ok, xi, 0), ok


def mcat_lliks(x, mask, V, logp, flags=0):
    """``ll[t, k] = s``: s starts at +0.0 and receives one plain add of ``logp[k, off_d + x_td]`` per present
    column in ascending d; all zeros for a row masked under MASK_AS_NAN.  x [n, D], logp [K, F]."""
    x = np.asarray(x, dtype=np.float64)
    logp = np.asarray(logp, dtype=np.float64)
    off = offsets_of(V)
    xi, ok = present(x, V)
    if (flags & MASK_AS_NAN) and mask is not None:
        ok = ok & ~np.asarray(mask, dtype=bool)[:, None]
    ll = np.zeros((x.shape[0], logp.shape[0]))
    for d in range(x.shape[1]):
        add = logp[:, off[d] + xi[:, d]].T              # [n, K]
        ll = np.where(ok[:, d][:, None], ll + add, ll)
    return ll


def mcat_counts(x, mask, V, q):
    """``counts[k, off_d + v] = sum q[t, k]`` over rows with ``mask[t] == 0`` whose entry d is present with
    symbol v.  x [n, D], q [n, K] -> [K, F]."""
    x = np.asarray(x, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    off = offsets_of(V)
    xi, ok = present(x, V)
    if mask is not None:
        ok = ok & ~np.asarray(mask, dtype=bool)[:, None]
    out = np.zeros((q.shape[1], int(off[-1])))
    for d in range(x.shape[1]):
        r = ok[:, d]
        np.add.at(out.T, off[d] + xi[r, d], q[r])
    return out


def window_rows(starts, Lm):
    return (np.asarray(starts, dtype=np.int64)[:, None] + np.arange(Lm)[None, :]).ravel()


def make_data(T, V, rng, mask_frac=0.1):
    """Symbol matrix [T, D] with every kind of entry the contract names: single NaN entries, whole NaN rows, a
    row whose every column is absent (mixed NaN / out of range), masked rows, one entry equal to V[d], one
    negative entry."""
    D = len(V)
    x = np.stack([rng.integers(0, v, size=T) for v in V], axis=1).astype(np.float64)
    mask = rng.random(T) < mask_frac
    if T >= 8:
        x[rng.random((T, D)) < 0.05] = np.nan
        x[rng.random(T) < 0.04] = np.nan
        r = rng.permutation(T)[:4]
        x[r[0]] = np.nan
        x[r[1]] = [V[d] if d % 2 else np.nan for d in range(D)]       # every column absent
        x[r[1], 0] = -1.0
        x[r[2], D - 1] = float(V[D - 1])                              # one past the last symbol
        x[r[3], 0] = -3.0
        mask[r[2]] = mask[r[3]] = False
        mask[r[0]] = True
    return x, mask


def make_model(K, V, rng):
    """(logp [K, F], mod_init [K], ltran [K, K]) of a random model, through digamma as the classes form them."""
    from scipy.special import digamma
    tabs = []
    for v in V:
        a = rng.random((K, v)) * 4 + 0.3
        tabs.append(digamma(a) - digamma(a.sum(1))[:, None])
    vt = 1.0 + rng.random((K, K)) * 20
    ltran = digamma(vt) - digamma(vt.sum(1))[:, None]
    vi = rng.random(K) + 0.1
    return np.concatenate(tabs, axis=1), digamma(vi) - digamma(vi.sum()), ltran


def split_tables(logp, V):
    off = offsets_of(V)
    return [np.ascontiguousarray(logp[:, off[d]:off[d + 1]]) for d in range(len(V))]


# ---- the problems the GPU tests and tools/ab_columns.py share
# K = 3: one ragged state tile; (16, 7 x 3): F = 21, no multiple of 16; 65: a second state group of one state, a
# one-symbol column; 256 with F = 96: the table beyond 64 KB (read through L2), four state groups; (16, 13 x 20): F = 260,
# four feature tiles per wave and a second feature group of four features, the 33 KB table staged
SHAPES = [(3, (2, 5)), (16, (3,) * 7), (64, (2,) * 12), (65, (4, 1, 7)), (256, (8,) * 12), (16, (20,) * 13)]
IDS = ["K3", "K16", "K64", "K65", "K256", "F260"]
T = 700
LENGTHS = (1, 2, 63, 64, 65, 257, 1)
_cache = {}


def problem(i):
    if i not in _cache:
        K, V = SHAPES[i]
        rng = np.random.default_rng(100 + i)
        x, mask = make_data(T, V, rng)
        logp, mod_init, ltran = make_model(K, V, rng)
        _cache[i] = dict(K=K, V=V, x=x, mask=mask, logp=logp, mod_init=mod_init, ltran=ltran)
    return _cache[i]
