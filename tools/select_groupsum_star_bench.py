"""Times the fused select-cascade + GROUP BY sums operator over a star join
(gdk.select_groupsum_star) against the same request through the operators
(mgdk_select_groupsum_star_opatatime) and against the fact-only hashed entry
in one process.

    python tools/select_groupsum_star_bench.py [rows]      -> one JSON object on stdout

Fact table: gdk.tpch_lineitem(1, 0, rows, 20000), rows default 60M, plus three
join indexes drawn uniformly at random (no nil oids) into generated
dimensions, Star Schema Benchmark sized:

    date      2 556 rows   year (int, 7 values)
    supplier  40 000 rows  nation (sht, 25 values), region (bte, 5 values)
    part      1 000 000 rows  category (int, 25 values), brand (sht, 250 values)

Every shape keeps Q1's predicate on shipdate (a fact column, read whole) and
sums price * (100 - discount) and quantity:

    date_key7            GROUP BY date.year
    date_pred_supp_key25 date.year = 1997, GROUP BY supplier.nation
    supp_pred_date_key7  supplier.region = 2, GROUP BY date.year
    supp_date_key175     GROUP BY supplier.nation, date.year
    part_pred_date_key7  part.category < 5, GROUP BY date.year
    part_key250          GROUP BY part.brand

Legs: "star_fused"; "star_opatatime", the operators; "hash_floor", the
fact-only hashed entry (gdk.select_groupsum_hash) on the same cascade with
every gathered column replaced by that column materialised at the fact
table's length beforehand -- what the request costs without the gather.  Per
shape each leg is warmed once; then --reps rounds (at least 7) run the legs in
turn, each call timed to its gdk.sync() ("samples_ms", "ms" their median,
"min_ms" / "max_ms" the spread).  The legs' results are checked to be equal,
group by group, before anything is printed.  "fused_below_operators_fastest"
says whether the fused median lies below the operators' fastest round;
"star_default" whether it does for every shape.
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


def mkdate(y, m, d):
    """MonetDB's date encoding (gdk_time.c): (year + 4712) * 12 + month - 1 in the bits above the day's five."""
    return (((y + 4712) * 12 + (m - 1)) << 5) | d


def join_index(rng, n, dim_rows):
    """n oids of a dimension of dim_rows rows, generated in pieces to bound the host memory in flight."""
    out = np.empty(n, np.uint64)
    step = 1 << 26
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        out[lo:hi] = rng.integers(0, dim_rows, hi - lo, dtype=np.uint64)
    return gdk.BAT.from_numpy(gdk.TYPE_oid, out, sorted_=False, revsorted=False, key=False, nonil=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rows", nargs="?", type=int, default=60_000_000)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    n, reps = args.rows, max(7, args.reps)
    gdk.init(0)
    c = gdk.tpch_lineitem(1, 0, n, 20_000)
    rng = np.random.default_rng(13)
    nd, ns, npart = 2_556, 40_000, 1_000_000
    col = (lambda tp, v: gdk.BAT.from_numpy(tp, v, sorted_=False, revsorted=False, key=False, nonil=True))
    dims = {"year": col(gdk.TYPE_int, (1992 + np.arange(nd) // 366).astype(np.int32)),
            "nation": col(gdk.TYPE_sht, rng.integers(0, 25, ns).astype(np.int16)),
            "region": col(gdk.TYPE_bte, rng.integers(0, 5, ns).astype(np.int8)),
            "category": col(gdk.TYPE_int, rng.integers(0, 25, npart).astype(np.int32)),
            "brand": col(gdk.TYPE_sht, rng.integers(0, 250, npart).astype(np.int16))}
    via = {"year": join_index(rng, n, nd)}
    via["nation"] = via["region"] = join_index(rng, n, ns)
    via["category"] = via["brand"] = join_index(rng, n, npart)
    # every dimension column at the fact table's length: the floor leg's columns
    flat = {k: gdk.BATproject(via[k], d) for k, d in dims.items()}
    ship = (c["shipdate"], mkdate(1998, 9, 2), "<=")
    sums = [(c["extendedprice"], ("-", 100, c["discount"])), (c["quantity"],)]
    shapes = {"date_key7": ([], ["year"]),
              "date_pred_supp_key25": ([("year", 1997, "==")], ["nation"]),
              "supp_pred_date_key7": ([("region", 2, "==")], ["year"]),
              "supp_date_key175": ([], ["nation", "year"]),
              "part_pred_date_key7": ([("category", 5, "<")], ["year"]),
              "part_key250": ([], ["brand"])}

    def rows_of(groups):
        return sorted((g["keys"], g["count"], g["first"], tuple(g["sums"])) for g in groups)

    def run_shape(dpreds, keys):
        used = [p[0] for p in dpreds] + keys
        vias = [(dims[k], via[k]) for k in used]

        def request(cols):
            return [ship] + [(cols[p[0]],) + p[1:] for p in dpreds], [cols[k] for k in keys], sums

        def star():
            groups, fused = gdk.select_groupsum_star(*request(dims), vias, fused=True)
            assert fused, "the star fused operator declared the request not applicable"
            return (rows_of(groups), {"lines": gdk.select_groupsum_star_last_lines(),
                                      "gathers": gdk.select_groupsum_star_last_gathers()})

        def operators():
            return rows_of(gdk.select_groupsum_star(*request(dims), vias, fused=False)[0]), {}

        def floor():
            groups, fused = gdk.select_groupsum_hash(*request(flat), fused=True)
            assert fused
            return rows_of(groups), {"lines": gdk.select_groupsum_hash_last_lines()}

        legs = {"star_fused": star, "star_opatatime": operators, "hash_floor": floor}
        results, info, ms = {}, {}, {k: [] for k in legs}
        for k, call in legs.items():
            results[k], info[k] = call()
            gdk.sync()
        for _ in range(reps):
            for k, call in legs.items():
                t = time.perf_counter()
                call()
                gdk.sync()
                ms[k].append(round((time.perf_counter() - t) * 1e3, 3))
        ref = results["star_fused"]
        assert all(r == ref for r in results.values()), "the legs disagree"
        out = {"groups": len(ref), "legs": {}}
        for k in legs:
            out["legs"][k] = dict(info[k], ms=float(np.median(ms[k])), min_ms=min(ms[k]), max_ms=max(ms[k]),
                                  samples_ms=ms[k])
        g, ops = out["legs"]["star_fused"]["ms"], out["legs"]["star_opatatime"]
        out["opatatime_over_fused"] = round(ops["ms"] / g, 3)
        out["fused_over_floor"] = round(g / out["legs"]["hash_floor"]["ms"], 3)
        out["fused_below_operators_fastest"] = g < ops["min_ms"]
        return out

    out = {"rows": n, "reps": reps, "shapes": {}}
    for k, v in shapes.items():
        print("select_groupsum_star_bench:", k, file=sys.stderr, flush=True)
        out["shapes"][k] = run_shape(*v)
    out["star_default"] = all(s["fused_below_operators_fastest"] for s in out["shapes"].values())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
