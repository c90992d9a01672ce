"""Times TPC-H Q6 three ways in one process: the general
fused select-cascade + SUM operator (gdk.select_sum), the same request
through the operators (mgdk_select_sum_opatatime) and the hand-tuned
mgdk_q6_fused.

    python tools/select_sum_bench.py [rows]      -> one JSON object on stdout

Input: gdk.tpch_lineitem(1, 0, rows, 20000), rows default 60M.  Each leg is
warmed once; then --reps rounds run the three legs in turn, each call timed
to its gdk.sync() ("samples_ms", "ms" their median).  "bytes" is what the
leg's kernel read by its own count -- the first predicate's column whole
plus 128 bytes per line of the later columns -- and "frac_8TBs" those bytes
over ms against 8 TB/s; the operator leg has no such count.  The three
results are checked to be equal before anything is printed.
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
    n = args.rows
    gdk.init(0)
    c = gdk.tpch_lineitem(1, 0, n, 20_000)
    d0, d1 = mkdate(1994, 1, 1), mkdate(1995, 1, 1)
    preds = [(c["shipdate"], d0, d1, True, False, False), (c["discount"], 5, 7, True, True, False),
             (c["quantity"], 2400, "<")]
    sums = [(c["extendedprice"], c["discount"])]
    first_bytes = n * 4                  # shipdate, read whole and raw by the general kernel

    def general():
        vals, _, used = gdk.select_sum(preds, sums, fused=True)
        assert used, "the fused operator declared Q6 not applicable"
        return vals[0], first_bytes + 128 * gdk.select_sum_last_lines()

    def operators():
        return gdk.select_sum(preds, sums, fused=False)[0][0], None

    def q6():
        r = gdk.q6_fused(c["shipdate"], c["discount"], c["quantity"], c["extendedprice"], d0, d1, 5, 7, 2400)
        return r, gdk.q6_last_bytes()

    legs = {"select_sum_fused": general, "select_sum_opatatime": operators, "q6_fused": q6}
    results, nbytes, ms = {}, {}, {k: [] for k in legs}
    for k, call in legs.items():
        results[k], nbytes[k] = call()
        gdk.sync()
    for _ in range(args.reps):
        for k, call in legs.items():
            t = time.perf_counter()
            call()
            gdk.sync()
            ms[k].append(round((time.perf_counter() - t) * 1e3, 3))
    assert len(set(results.values())) == 1, results
    out = {"rows": n, "reps": args.reps, "revenue": str(results["q6_fused"]), "legs": {}}
    for k in legs:
        med = float(np.median(ms[k]))
        d = {"ms": med, "samples_ms": ms[k], "bytes": nbytes[k]}
        if nbytes[k] is not None:
            d["frac_8TBs"] = round(nbytes[k] / (med * 1e-3) / PEAK, 4)
        out["legs"][k] = d
    g = out["legs"]["select_sum_fused"]["ms"]
    out["opatatime_over_fused"] = round(out["legs"]["select_sum_opatatime"]["ms"] / g, 3)
    out["fused_over_q6_fused"] = round(g / out["legs"]["q6_fused"]["ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
