"""Times TPC-H Q1 three ways in one process: the general
fused select-cascade + GROUP BY sums operator (gdk.select_groupsum), the same
request through the operators (mgdk_select_groupsum_opatatime) and the
hand-tuned mgdk_q1_fused.

    python tools/select_groupsum_bench.py [rows]      -> one JSON object on stdout

Input: gdk.tpch_lineitem(1, 0, rows, 20000), rows default 60M.  Each leg is
warmed once; then --reps rounds (at least 7) run the three legs in turn, each
call timed to its gdk.sync() ("samples_ms", "ms" their median, "min_ms" /
"max_ms" the spread).  "bytes" is what the general kernel read by its own
count -- the first predicate's column whole plus 128 bytes per line of the
later columns; the other legs have no such count.  The three results are
checked to be equal, group by group, before anything is printed.
"fused_below_operators_fastest" says whether the fused median lies below the
operators' fastest round.
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
    keys = [c["returnflag"], c["linestatus"]]
    qty, price, disc, tax = c["quantity"], c["extendedprice"], c["discount"], c["tax"]
    sums = [(qty,), (price,), (price, ("-", 100, disc)), (price, ("-", 100, disc), ("+", 100, tax)), (disc,)]
    first_bytes = n * 4                  # shipdate, read whole

    def rows_of(groups):
        return sorted((g["keys"], g["count"], g["first"], tuple(g["sums"])) for g in groups)

    def general():
        groups, used = gdk.select_groupsum(preds, keys, sums, fused=True)
        assert used, "the fused operator declared Q1 not applicable"
        return rows_of(groups), first_bytes + 128 * gdk.select_groupsum_last_lines()

    def operators():
        return rows_of(gdk.select_groupsum(preds, keys, sums, fused=False)[0]), None

    def q1():
        r = gdk.q1_fused(c, dmax)
        return sorted(((x["returnflag"], x["linestatus"]), x["count_order"], x["first_row"],
                       (x["sum_qty"], x["sum_base_price"], x["sum_disc_price"], x["sum_charge"], x["sum_disc"]))
                      for x in r), None

    legs = {"select_groupsum_fused": general, "select_groupsum_opatatime": operators, "q1_fused": q1}
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
    assert results["select_groupsum_fused"] == results["select_groupsum_opatatime"] == results["q1_fused"], results
    out = {"rows": n, "reps": reps, "groups": len(results["q1_fused"]),
           "sum_charge": [str(r[3][3]) for r in results["q1_fused"]], "legs": {}}
    for k in legs:
        med = float(np.median(ms[k]))
        d = {"ms": med, "min_ms": min(ms[k]), "max_ms": max(ms[k]), "samples_ms": ms[k], "bytes": nbytes[k]}
        if nbytes[k] is not None:
            d["frac_8TBs"] = round(nbytes[k] / (med * 1e-3) / PEAK, 4)
        out["legs"][k] = d
    g = out["legs"]["select_groupsum_fused"]["ms"]
    out["opatatime_over_fused"] = round(out["legs"]["select_groupsum_opatatime"]["ms"] / g, 3)
    out["fused_over_q1_fused"] = round(g / out["legs"]["q1_fused"]["ms"], 3)
    out["fused_below_operators_fastest"] = g < out["legs"]["select_groupsum_opatatime"]["min_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
