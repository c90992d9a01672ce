"""Times the hashed fused select-cascade + GROUP BY sums operator
(gdk.select_groupsum_hash) against the same request through the operators
(mgdk_select_groupsum_hash_opatatime) in one process.

    python tools/select_groupsum_hash_bench.py [rows]      -> one JSON object on stdout

Input: gdk.tpch_lineitem(1, 0, rows, 20000), rows default 60M, with Q1's
predicate and Q1's five sums, grouped four ways:

    int7         one int key, 7 values, uniformly random
    sht_int175   a sht key of 25 values and an int key of 7: 175 groups
    lng256       one lng key, 256 random 64-bit values, uniformly random
    q1           Q1 itself (two str flags of one byte): the hashed entry beside
                 the narrow entry (gdk.select_groupsum) and mgdk_q1_fused

Per shape each leg is warmed once; then --reps rounds (at least 7) run the
legs in turn, each call timed to its gdk.sync() ("samples_ms", "ms" their
median, "min_ms" / "max_ms" the spread).  "bytes" is what the hashed kernel
read by its own count -- the first predicate's column whole plus 128 bytes per
line of the later columns.  The legs' results are checked to be equal, group
by group, before anything is printed.  "fused_below_operators_fastest" says
whether the fused median lies below the operators' fastest round.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monetdb_amd import gdk  # noqa: E402

PEAK = 8e12


def mkdate(y, m, d):
    """MonetDB's date encoding (gdk_time.c): (year + 4712) * 12 + month - 1 in the bits above the day's five."""
    return (((y + 4712) * 12 + (m - 1)) << 5) | d


def random_key(rng, n, values, tp):
    """n draws from `values`, generated in pieces to bound the host memory in flight."""
    values = np.asarray(values)
    out = np.empty(n, values.dtype)
    step = 1 << 26
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        out[lo:hi] = values[rng.integers(0, len(values), hi - lo)]
    return gdk.BAT.from_numpy(tp, out, sorted_=False, revsorted=False, key=False, nonil=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rows", nargs="?", type=int, default=60_000_000)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    n, reps = args.rows, max(7, args.reps)
    gdk.init(0)
    c = gdk.tpch_lineitem(1, 0, n, 20_000)
    dmax = mkdate(1998, 9, 2)
    preds = [(c["shipdate"], dmax, "<=")]
    qty, price, disc, tax = c["quantity"], c["extendedprice"], c["discount"], c["tax"]
    sums = [(qty,), (price,), (price, ("-", 100, disc)), (price, ("-", 100, disc), ("+", 100, tax)), (disc,)]
    first_bytes = n * 4                  # shipdate, read whole
    rng = np.random.default_rng(12)

    def rows_of(groups):
        return sorted((g["keys"], g["count"], g["first"], tuple(g["sums"])) for g in groups)

    def run_shape(keys, extra=None):
        def fused():
            groups, used = gdk.select_groupsum_hash(preds, keys, sums, fused=True)
            assert used, "the hashed fused operator declared the request not applicable"
            return rows_of(groups), first_bytes + 128 * gdk.select_groupsum_hash_last_lines()

        def operators():
            return rows_of(gdk.select_groupsum_hash(preds, keys, sums, fused=False, maxgroups=256)[0]), None

        legs = {"select_groupsum_hash_fused": fused, "select_groupsum_hash_opatatime": operators}
        legs.update(extra or {})
        results, nbytes, ms = {}, {}, {k: [] for k in legs}
        for k, call in legs.items():
            results[k], nbytes[k] = call()
            gdk.sync()
        for _ in range(reps):
            for k, call in legs.items():
                t = time.perf_counter()
                call()
                gdk.sync()
                ms[k].append(round((time.perf_counter() - t) * 1e3, 3))
        ref = results["select_groupsum_hash_fused"]
        assert all(r == ref for r in results.values()), "the legs disagree"
        out = {"groups": len(ref), "legs": {}}
        for k in legs:
            med = float(np.median(ms[k]))
            d = {"ms": med, "min_ms": min(ms[k]), "max_ms": max(ms[k]), "samples_ms": ms[k], "bytes": nbytes[k]}
            if nbytes[k] is not None:
                d["frac_8TBs"] = round(nbytes[k] / (med * 1e-3) / PEAK, 4)
            out["legs"][k] = d
        g = out["legs"]["select_groupsum_hash_fused"]["ms"]
        ops = out["legs"]["select_groupsum_hash_opatatime"]
        out["opatatime_over_fused"] = round(ops["ms"] / g, 3)
        out["fused_below_operators_fastest"] = g < ops["min_ms"]
        return out

    out = {"rows": n, "reps": reps, "shapes": {}}
    year = random_key(rng, n, np.arange(1992, 1999, dtype=np.int32), gdk.TYPE_int)
    out["shapes"]["int7"] = run_shape([year])
    nation = random_key(rng, n, np.arange(25, dtype=np.int16), gdk.TYPE_sht)
    out["shapes"]["sht_int175"] = run_shape([nation, year])
    del nation, year
    wide = random_key(rng, n, rng.integers(-(1 << 63), (1 << 63) - 1, 256, dtype=np.int64), gdk.TYPE_lng)
    out["shapes"]["lng256"] = run_shape([wide])
    del wide
    flags = [c["returnflag"], c["linestatus"]]

    def narrow():
        groups, used = gdk.select_groupsum(preds, flags, sums, fused=True)
        assert used
        return rows_of(groups), first_bytes + 128 * gdk.select_groupsum_last_lines()

    def q1():
        r = gdk.q1_fused(c, dmax)
        return sorted(((x["returnflag"], x["linestatus"]), x["count_order"], x["first_row"],
                       (x["sum_qty"], x["sum_base_price"], x["sum_disc_price"], x["sum_charge"], x["sum_disc"]))
                      for x in r), None

    out["shapes"]["q1"] = run_shape(flags, {"select_groupsum_fused": narrow, "q1_fused": q1})
    out["hashed_default"] = all(s["fused_below_operators_fastest"] for s in out["shapes"].values())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
