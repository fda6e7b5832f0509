"""NumPy statements of the two held-out formulas (svihmm_heldout_rows / svihmm_heldout_entries, include/svihmm.h),
the entry lists and the problems the CPU and the GPU tests share.  Host-side only.

    lp = LSE_k( log(q[g, k] + 1e-9) + term_k )

row mode: term = the family's llik of the row's true values; entry mode: term of ONE entry (g, d, x) of a product
family, in the operation order the header fixes.  LSE here is the max-shifted form  m + log(sum exp(v - m))  -- the
form the kernel uses, with K roundings of size ulp(1) in the sum instead of logaddexp.reduce's K roundings of size
ulp(|v|)."""
import numpy as np

from oracle import ref_numpy as R
from tests import mcat_helpers as MH
from tests import poisson_helpers as PH

MASK_AS_NAN = 1
EPS = 1e-9
PER_BLOCK = 2048          # entries / rows per workgroup of the two kernels (HELDOUT_PER_BLOCK)


def lse_rows(v):
    m = np.max(v, axis=1)
    return m + np.log(np.sum(np.exp(v - m[:, None]), axis=1))


# ---- the families' models as one dict each -------------------------------------------------------------------------
def poisson_problem(i):
    p = dict(PH.problem(i))
    p["fam"] = "poisson"
    return p


# K of the Poisson shapes; V mixes columns of 1, 2 and 7 symbols; the last case has D = 128 and sum V = 1024 (the limits)
MCAT_K = [3, 16, 64, 65, 256, 16]
MCAT_V = [[1, 2, 7], [7, 1, 2, 2, 7, 1, 7], [2, 7, 1] * 4, [7, 2, 1], [1, 7, 2, 7, 7, 2, 1, 2],
          [1, 2, 7] * 41 + [7, 200, 200, 200, 7]]
MCAT_IDS = ["K3", "K16", "K64", "K65", "K256", "F1024"]
T = PH.T
_mcat = {}


def mcat_problem(i):
    if i not in _mcat:
        K, V = MCAT_K[i], MCAT_V[i]
        rng = np.random.default_rng(900 + i)
        logp, mod_init, ltran = MH.make_model(K, V, rng)
        x, mask = MH.make_data(T, V, rng)
        _mcat[i] = dict(fam="mcat", K=K, D=len(V), V=list(V), logp=logp, mod_init=mod_init, ltran=ltran, x=x, mask=mask)
    return _mcat[i]


def problem(fam, i):
    return poisson_problem(i) if fam == "poisson" else mcat_problem(i)


def seq_problem(fam, i):
    """The first sum(LENGTHS) rows of a problem as sequences of poisson_helpers.LENGTHS: (problem, offsets, rows)."""
    p = dict(problem(fam, i))
    Ts = sum(PH.LENGTHS)
    p["x"], p["mask"] = p["x"][:Ts], p["mask"][:Ts]
    off = np.zeros(len(PH.LENGTHS) + 1, dtype=np.int64)
    np.cumsum(PH.LENGTHS, out=off[1:])
    return p, off, Ts


def lliks(p, x, mask, flags):
    if p["fam"] == "poisson":
        return PH.poisson_lliks(x, mask, p["elog"], p["erate"], p["logfact"], flags)
    return MH.mcat_lliks(x, mask, p["V"], p["logp"], flags)


def present(p, x):
    """(integer value, present) of entries x [n, D] under the family's rule."""
    return PH.present(x, p["C"]) if p["fam"] == "poisson" else MH.present(x, p["V"])


def entry_present(p, cols, vals):
    """(c int[n], ok bool[n]) of the entry list: the family's rule applied to vals[e] in column cols[e]."""
    cols = np.asarray(cols, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.float64)
    if p["fam"] == "poisson":
        c, ok = PH.present(vals[:, None], p["C"])
        return c[:, 0], ok[:, 0]
    nan = np.isnan(vals)
    with np.errstate(invalid="ignore"):
        xi = np.trunc(np.where(nan | np.isinf(vals), -1.0, vals)).astype(np.int64)
    ok = (~nan) & (xi >= 0) & (xi < np.asarray(p["V"], dtype=np.int64)[cols])
    return np.where(ok, xi, 0), ok


def entry_terms(p, cols, vals):
    """``(term [n, K], ok [n], M [n])``: term_k of every entry in the header's operation order (rows of absent entries
    hold zeros) and the largest magnitude among the operands of an entry's term (c elog, erate, logfact[c] / logp)."""
    cols = np.asarray(cols, dtype=np.int64)
    c, ok = entry_present(p, cols, vals)
    if p["fam"] == "poisson":
        elog, erate = p["elog"][:, cols].T, p["erate"][:, cols].T            # [n, K]
        lf = p["logfact"][c]
        t = c.astype(np.float64)[:, None] * elog         # one rounded multiply
        mag = np.maximum(np.abs(t).max(1), np.maximum(np.abs(erate).max(1), np.abs(lf)))
        t = t - erate
        t = t - lf[:, None]
    else:
        off = MH.offsets_of(p["V"])
        t = p["logp"][:, off[cols] + c].T
        mag = np.abs(t).max(1)
    return np.where(ok[:, None], t, 0.0), ok, np.where(ok, mag, 0.0)


def heldout_entries_numpy(p, q, rows, cols, vals):
    """``(lp [n], M [n])``: lp_e of every entry against the posterior rows q [nrows, K] (NaN for absent entries) and
    the magnitude M the kernel test's bound is built from (the entry's operands and log(q + 1e-9))."""
    rows = np.asarray(rows, dtype=np.int64)
    if len(rows) == 0:
        return np.empty(0), np.empty(0)
    term, ok, mag = entry_terms(p, cols, vals)
    lq = np.log(q[rows] + EPS)
    lp = lse_rows(lq + term)
    return np.where(ok, lp, np.nan), np.maximum(mag, np.abs(lq).max(1))


def heldout_rows_numpy(q, ll_true, masked):
    """lp [nrows]: LSE_k(log(q + 1e-9) + ll_true) for the masked batch rows, NaN elsewhere."""
    lp = lse_rows(np.log(q + EPS) + ll_true)
    return np.where(np.asarray(masked, dtype=bool), lp, np.nan)


def mean_count(lp):
    ok = ~np.isnan(lp)
    n = int(ok.sum())
    return (float(np.mean(lp[ok])) if n else None), n


def kernel_order_mean(lp):
    """The mean as the kernels form it: entry e belongs to workgroup e // PER_BLOCK and there to the 16-lane row
    (e % PER_BLOCK) % 16, which adds its entries in ascending e; the 16 rows' sums are added in row order, the
    workgroups' partials in workgroup order."""
    tot, cnt = 0.0, 0
    for b0 in range(0, len(lp), PER_BLOCK):
        blk = lp[b0:b0 + PER_BLOCK]
        a = 0.0
        for rg in range(16):
            s = 0.0
            for v in blk[rg::16]:
                if not np.isnan(v):
                    s += float(v)
                    cnt += 1
            a += s
        tot += a
    return (tot / cnt if cnt else None), cnt


def referee_posterior(ll, mod_init, ltran):
    return R.posterior(R.forward_msgs(ll, mod_init, ltran), R.backward_msgs(ll, ltran))


# ---- entry lists -----------------------------------------------------------------------------------------------------
def absent_values(p, d):
    """One value of each absent kind the family defines, for column d."""
    if p["fam"] == "poisson":
        return [np.nan, -1.0, -0.5, np.inf, float(p["C"] + 1)]
    return [np.nan, -1.0, float(p["V"][d])]


def top_value(p, d):
    """The largest present value of column d: C for the counts, V[d] - 1 for the symbols."""
    return float(p["C"]) if p["fam"] == "poisson" else float(p["V"][d] - 1)


def entry_list(p, x_batch, n_speckle, seed):
    """Entries against a batch whose rows hold the values x_batch [nrows, D]:
    ``(rows int64[n], cols int32[n], vals[n], n_speckle)``.  First n_speckle speckled entries, drawn without
    replacement among the present entries of x_batch with their true values (the ones a test blanks before the
    E-step); then two duplicates of speckled entries, one entry of each absent kind, one entry equal to the top
    value (C for counts: present), one in column D - 1 and one in the last batch row."""
    rng = np.random.default_rng(seed)
    nrows, D = x_batch.shape
    _, ok = present(p, x_batch)
    flat = np.flatnonzero(ok)
    n_speckle = min(n_speckle, flat.size)
    pick = np.sort(rng.choice(flat, size=n_speckle, replace=False))
    r, c = np.divmod(pick, D)
    v = x_batch[r, c]
    rows, cols, vals = list(r), list(c), list(v)
    for e in (0, n_speckle // 2):
        rows.append(r[e]); cols.append(c[e]); vals.append(v[e])
    d0 = int(rng.integers(0, D))
    for a in absent_values(p, d0):
        rows.append(int(rng.integers(0, nrows))); cols.append(d0); vals.append(a)
    d1 = int(rng.integers(0, D))
    rows.append(int(rng.integers(0, nrows))); cols.append(d1); vals.append(top_value(p, d1))
    rows.append(int(rng.integers(0, nrows))); cols.append(D - 1); vals.append(0.0)
    rows.append(nrows - 1); cols.append(int(rng.integers(0, D))); vals.append(0.0)
    return (np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int32), np.asarray(vals, dtype=np.float64),
            n_speckle)


def window_rows(starts, Lm):
    return PH.window_rows(starts, Lm)


# ---- the end-to-end cases: a batch kind on a problem, entries blanked, the referee's posteriors -----------------------
KINDS = ("windows", "chain", "sequences", "subset")
WINDOW_STARTS, WINDOW_LM = np.array([0, 25, 50, 330, 660], dtype=np.int64), 40      # the first three overlap
SUBSET_IDX = np.array([5, 2, 5, 3], dtype=np.int32)                                  # sequence 5 twice
N_SPECKLE = 200
_cases = {}


def batch_layout(kind, off=None):
    """``(resident row of every batch row, [(first batch row, length) of every chain])`` of a batch kind."""
    if kind == "windows":
        res = window_rows(WINDOW_STARTS, WINDOW_LM)
        return res, [(b * WINDOW_LM, WINDOW_LM) for b in range(len(WINDOW_STARTS))]
    if kind == "chain":
        return np.arange(T, dtype=np.int64), [(0, T)]
    if kind == "sequences":
        return np.arange(int(off[-1]), dtype=np.int64), [(int(a), int(b - a)) for a, b in zip(off[:-1], off[1:])]
    lens = (off[SUBSET_IDX + 1] - off[SUBSET_IDX]).astype(np.int64)
    dst = np.concatenate(([0], np.cumsum(lens)))
    res = np.concatenate([np.arange(off[s], off[s + 1]) for s in SUBSET_IDX]).astype(np.int64)
    return res, [(int(dst[m]), int(lens[m])) for m in range(len(lens))]


def e2e_case(fam, i, kind):
    """One end-to-end case: dict with the problem ``p``, the sequence offsets ``off`` (None for the window kinds),
    ``res`` (resident row of every batch row), the entry list ``rows`` (batch rows) / ``cols`` / ``vals``, ``xb`` (the
    resident data with the speckled entries blanked), ``q`` (the NumPy referee's posteriors of the batch rows, E-step
    on ``xb`` with the masked rows missing), ``ll_true`` (lliks of the batch rows' resident values, nothing masked)
    and ``masked`` (the batch rows' mask bytes).  Computed once per case and left unchanged."""
    key = (fam, i, kind)
    if key not in _cases:
        off = None
        if kind in ("sequences", "subset"):
            p, off, _ = seq_problem(fam, i)
        else:
            p = problem(fam, i)
        res, chains = batch_layout(kind, off)
        rows, cols, vals, ns = entry_list(p, p["x"][res], N_SPECKLE, seed=1000 + 10 * i + KINDS.index(kind))
        xb = p["x"].copy()
        xb[res[rows[:ns]], cols[:ns]] = np.nan
        ll = lliks(p, xb[res], p["mask"][res], MASK_AS_NAN)
        q = np.concatenate([referee_posterior(ll[a:a + n], p["mod_init"], p["ltran"]) for a, n in chains])
        _cases[key] = dict(p=p, off=off, res=res, chains=chains, rows=rows, cols=cols, vals=vals, ns=ns, xb=xb, q=q,
                           ll=ll, ll_true=lliks(p, xb[res], None, 0), masked=p["mask"][res].astype(bool))
    return _cases[key]
