"""Times the ranking window functions (SQLrow_number, SQLrank, SQLdense_rank,
SQLpercent_rank, SQLcume_dist) over partition / peer bit
columns of four layouts, with GDKanalyticalntile on the same partition bits
beside them: it stands for the compacted-starts design (segments.h) that the
ranking functions avoid.

    python tools/window_rank_bench.py [rows]      -> one JSON object on stdout

Layouts (rows default 100M):
    unique_key        no p, every row a peer start
    4_parts           4 partitions, peer groups of 16 rows
    1e5_parts         10^5 partitions, peer groups of 16 rows
    parts_of_10       rows / 10 partitions of 10 rows, every row a peer start

Per leg: a warm-up call, gdk.sync(), then --reps calls timed one by one
("samples_ms", "ms" their median); "device_ms" is the entry point's mean time
between its two stream events (mgdk_prof_get) over the same calls;
"bytes_per_row" is what the kernels of that call read and write by their own
count (p and o twice each, the result once; the tile state is 20 bytes per
4096 rows and left out), "frac_8TBs" that traffic over ms against 8 TB/s.
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
PROF = {"row_number": "sqlrow_number", "rank": "sqlrank", "dense_rank": "sqldense_rank",
        "percent_rank": "sqlpercent_rank", "cume_dist": "sqlcume_dist", "ntile": "analyticalntile"}


def layouts(n):
    i = np.arange(n, dtype=np.int64)
    ones = np.ones(n, np.int8)
    yield "unique_key", None, ones
    for name, parts in (("4_parts", 4), ("1e5_parts", 100_000)):
        plen = (n + parts - 1) // parts
        p = (i % max(plen, 1) == 0).astype(np.int8)
        yield name, p, np.maximum(p, (i % 16 == 0).astype(np.int8))
    yield "parts_of_10", (i % 10 == 0).astype(np.int8), ones


def bytes_per_row(fn, has_p, has_o):
    """the traffic of one call by the kernels' own count"""
    if fn == "ntile":
        return None          # starts list and search: not a streaming count
    out = 8 if fn in ("percent_rank", "cume_dist") else 4
    if fn == "row_number":
        return out + (2 if has_p else 0)
    if not has_o:
        return out           # a fill: nothing is read
    return out + 2 + (2 if has_p else 0)


def leg(fn, call, reps, n, bpr):
    call()
    gdk.sync()
    gdk.prof_reset()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        gdk.sync()
        ms.append(round((time.perf_counter() - t) * 1e3, 3))
    dev, launches = gdk.prof_get(PROF[fn])
    d = {"ms": float(np.median(ms)), "samples_ms": ms,
         "device_ms": round(dev / launches, 3) if launches else None}
    if bpr is not None:
        d["bytes_per_row"] = bpr
        d["frac_8TBs"] = round(bpr * n / (d["ms"] * 1e-3) / PEAK, 4)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rows", nargs="?", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    n = args.rows
    gdk.init(0)
    gdk.prof_enable(True)
    b = gdk.BAT.dense(0, n)
    res = {"rows": n, "reps": args.reps, "layouts": {}}
    for name, p, o in layouts(n):
        P = gdk.BAT.from_numpy(gdk.TYPE_bit, p) if p is not None else None
        O = gdk.BAT.from_numpy(gdk.TYPE_bit, o)
        legs = {
            "row_number": lambda: gdk.SQLrow_number(b, P),
            "rank": lambda: gdk.SQLrank(b, P, O),
            "dense_rank": lambda: gdk.SQLdense_rank(b, P, O),
            "percent_rank": lambda: gdk.SQLpercent_rank(b, P, O),
            "cume_dist": lambda: gdk.SQLcume_dist(b, P, O),
            "ntile": lambda: gdk.GDKanalyticalntile(b, P, ntile=4, tpe=gdk.TYPE_int),
        }
        out = {}
        for fn, call in legs.items():
            out[fn] = leg(fn, call, args.reps, n, bytes_per_row(fn, P is not None, True))
            print(json.dumps({name: {fn: out[fn]}}), file=sys.stderr, flush=True)
        res["layouts"][name] = out
        del P, O
    print(json.dumps(res))


if __name__ == "__main__":
    main()
