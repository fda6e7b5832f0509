"""A/B of the column-wise families (multi-column Categorical, Poisson, Gaussian tracks) between two builds of the
library on one MI355X: the same bits, and the same speed.

    python tools/ab_columns.py --bits  build_exp/libsvihmm_parent.so  [--out profiles/columns_frame_ab.json]
    python tools/ab_columns.py --speed build_exp/libsvihmm_parent.so  [--pairs 8] [--out ...]

The library named is the A side (loaded through SVIHMM_HIP_LIB), the product the B side.  Every run is a child
process of its own under a time limit; the first child that fails or runs out of time ends the tool -- nothing else
is started on the device after it.
  --bits   one child per library runs the problems of the tests' builders (tests/mcat_helpers.py, poisson_helpers.py,
           pgauss_helpers.py: every shape; tests/svi_family_helpers.py: every case, three iterations of the resident
           loop) and dumps every array it reads back to a temporary .npz; the two dumps must hold the same bytes, name by name.
  --speed  the device child of the `windows` case of tools/bench_mcat.py, bench_poisson.py and bench_pgauss.py,
           alternating A and B; call_ms and the stats / emission entries of kernel_ms of every run.  A figure is
           accepted when B's median is not above A's by more than the standard deviation of A's runs.
--out merges the section written into the JSON file (the other sections stay).  Exit status 1: an array differs or a
speed figure is not accepted."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
SUFFSTATS_EDGES = [(1, 1), (3, 1), (2, 2), (1, 5), (9, 7), (1, 64), (5, 13)]      # 1, 3, 4, 5, 63, 64, 65 rows


def dump(path):
    import numpy as np
    from pysvihmm_amd import _lib as L
    from pysvihmm_amd.engine import HipEngine
    from tests import mcat_helpers as MH, pgauss_helpers as GH, poisson_helpers as PH, svi_family_helpers as SH
    out = {}
    eng = HipEngine(0)

    def stats(tag, st):
        out[tag] = st.buf.copy()

    def family(name, n, problem, push, T, lengths):
        for i in range(n):
            p = problem(i)
            push(eng, p)
            K = p["K"]
            starts = (np.arange(5) * 131) % (T - 37 + 1)
            for flags in (0, L.MASK_AS_NAN):
                out["%s%d/loglik/%d" % (name, i, flags)] = eng.loglik(starts, 37, flags=flags)
            for B, Lm in ((6, 37), (192, 16)):
                starts = np.tile((np.arange(min(B, 24)) * 29) % (T - Lm + 1), max(1, B // 24))
                for flags in (0, L.TRANS_WRAP, L.TRANS_WRAP | L.MASK_AS_NAN):
                    stats("%s%d/estep/%dx%d/%d" % (name, i, B, Lm, flags), eng.estep(starts, Lm, flags=flags))
            rng = np.random.default_rng(7 + i)
            for B, Lm in SUFFSTATS_EDGES:
                starts = (np.arange(B) * 97 + 11) % (T - Lm + 1)
                q = rng.dirichlet(np.ones(K), size=(B, Lm))
                q[rng.random((B, Lm)) < 0.2] = 0.0
                stats("%s%d/suffstats/%dx%d" % (name, i, B, Lm), eng.suffstats(starts, Lm, q, flags=0))
            Ts = sum(lengths)
            push(eng, p, p["x"][:Ts], p["mask"][:Ts])
            eng.set_sequences(lengths)
            st, seq_lb, q0 = eng.estep_sequences(flags=0)
            stats("%s%d/sequences/stats" % (name, i), st)
            out["%s%d/sequences/lb" % (name, i)], out["%s%d/sequences/q0" % (name, i)] = seq_lb, q0
            eng.set_sequences(None)

    def push_mcat(e, p, x=None, mask=None):
        e.set_obs(p["x"] if x is None else x, p["mask"] if mask is None else mask)
        e.set_globals(p["mod_init"], p["ltran"])
        e.set_emission_mcat(MH.split_tables(p["logp"], p["V"]))

    def push_pgauss(e, p, x=None, mask=None):
        e.set_emission_pgauss(p["mu"], p["hprec"], p["cst"], p["origin"])
        e.set_obs(p["x"] if x is None else x, p["mask"] if mask is None else mask)
        e.set_globals(p["mod_init"], p["ltran"])

    def push_poisson(e, p, x=None, mask=None):
        e.set_obs(p["x"] if x is None else x, p["mask"] if mask is None else mask)
        e.set_globals(p["mod_init"], p["ltran"])
        e.set_emission_poisson(p["elog"], p["erate"], p["C"])

    family("mcat", len(MH.SHAPES), MH.problem, push_mcat, MH.T, MH.LENGTHS)
    family("poisson", len(PH.SHAPES), PH.problem, push_poisson, PH.T, PH.LENGTHS)
    family("pgauss", len(GH.SHAPES), GH.problem, push_pgauss, GH.T, GH.LENGTHS)
    eng.close()
    for ci, spec in enumerate(SH.FAMILY_CASES):
        c = SH.family_case(*spec)
        eng = HipEngine(0)
        eng.set_obs(c["obs"], c["mask"])       # (case_begin with room for three iterations)
        if c["fam"] == "mcat":
            eng.svi_begin_mcat(c["prior_tran"], c["var_tran"], c["prior"], c["factors"], 3)
        else:
            eng.svi_begin_poisson(c["prior_tran"], c["var_tran"], c["prior"], c["factors"], SH.POIS_C, 3)
        if "adagrad" in c["opts"]:
            eng.svi_set_adagrad(np.ones((c["K"], c["K"])))
        for it in range(3):
            eng.svi_iteration(it, c["starts"][it % c["nit"]], c["B"], c["Lm"], L.TRANS_WRAP, c["rho"], c["bA"], c["bE"])
            tag = "svi%d/%s/it%d/" % (ci, SH.family_case_id(spec), it)
            out[tag + "packed"] = eng.read_packed().buf.copy()
            vt, vi, fac = eng.svi_read_factors()
            out[tag + "var_tran"], out[tag + "var_init"] = vt, vi
            for j, f in enumerate(fac):
                out[tag + "factor%d" % j] = f
        out["svi%d/elbo" % ci] = eng.svi_read_elbo(3)[0]
        eng.close()
    np.savez(path, **out)
    print("DUMPED %d arrays" % len(out), flush=True)


def child(cmd, lib, limit):
    env = dict(os.environ)
    if lib:
        env["SVIHMM_HIP_LIB"] = os.path.join(REPO, lib)
    try:
        p = subprocess.run([sys.executable] + cmd, cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit("ab_columns: %s (%s) ran past %d s; nothing more is started" % (cmd, lib or "product", limit))
    if p.returncode:
        sys.exit("ab_columns: %s (%s) ended with status %d; nothing more is started\n%s"
                 % (cmd, lib or "product", p.returncode, p.stderr[-3000:]))
    return p.stdout


def bits(lib, limit):
    import numpy as np
    with tempfile.TemporaryDirectory() as tmp:
        files = {}
        for side, l in (("A", lib), ("B", None)):
            files[side] = os.path.join(tmp, side + ".npz")
            print(side, child([os.path.abspath(__file__), "--dump", files[side]], l, limit).strip().splitlines()[-1], flush=True)
        a, b = np.load(files["A"]), np.load(files["B"])
        names = sorted(a.files)
        # (the same bytes: array_equal, and a NaN both sides hold at the same place is the same result)
        differing = [n for n in names if n not in b.files or a[n].shape != b[n].shape or a[n].tobytes() != b[n].tobytes()]
        res = {"A": lib, "B": "product", "arrays": len(names), "same_names": names == sorted(b.files),
               "elements": int(sum(a[n].size for n in names)), "differing": differing,
               "verdict": "all arrays equal" if not differing and names == sorted(b.files) else "DIFFERENT"}
    print(json.dumps(res), flush=True)
    return res


def speed(lib, pairs, limit, save):
    res = {"A": lib, "B": "product", "pairs": pairs, "families": {}}
    for fam in ("mcat", "poisson", "pgauss"):
        runs = {"A": {"call_ms": [], "stats": [], "emission": []}, "B": {"call_ms": [], "stats": [], "emission": []}}
        for rnd in range(pairs):
            for side, l in (("A", lib), ("B", None)):
                o = child([os.path.join(REPO, "tools", "bench_%s.py" % fam), "--case", "windows", "--route", "device"], l, limit)
                r = json.loads([x for x in o.splitlines() if x.startswith("RESULT ")][-1][7:])
                runs[side]["call_ms"].append(r["call_ms"])
                runs[side]["stats"].append(r["kernel_ms"]["stats"])
                runs[side]["emission"].append(r["kernel_ms"]["emission"])
                print(fam, rnd, side, r["call_ms"], r["kernel_ms"]["stats"], r["kernel_ms"]["emission"], flush=True)
        verdict = {}
        for key in ("call_ms", "stats", "emission"):
            ma, mb, sd = statistics.median(runs["A"][key]), statistics.median(runs["B"][key]), statistics.stdev(runs["A"][key])
            verdict[key] = {"median_A": ma, "median_B": mb, "stdev_A": sd, "accepted": mb - ma <= sd}
        res["families"][fam] = {"runs": runs, "verdict": verdict}
        print(fam, json.dumps(verdict), flush=True)
        save(res)                      # (a family's figures are on disk before the next one starts)
    missed = ["%s %s" % (fam, key) for fam, d in res["families"].items() for key, v in d["verdict"].items() if not v["accepted"]]
    res["verdict"] = "accepted" if not missed else "NOT ACCEPTED: " + ", ".join(missed)
    print("speed:", res["verdict"], flush=True)
    save(res)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump")
    ap.add_argument("--bits")
    ap.add_argument("--speed")
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.dump:
        dump(args.dump)
        return 0
    if not os.path.exists("/dev/kfd"):
        print("ab_columns: no GPU", file=sys.stderr)
        return 2
    doc = {}
    if args.out and os.path.exists(args.out):
        doc = json.load(open(args.out))

    def save(section, value):
        doc[section] = value
        if args.out:
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
    if args.bits:
        save("bits", bits(args.bits, args.limit))
    if args.speed:
        speed(args.speed, args.pairs, args.limit, lambda res: save("speed", res))
    ok = (doc.get("bits", {}).get("verdict", "all arrays equal") == "all arrays equal"
          and doc.get("speed", {}).get("verdict", "accepted") == "accepted")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
