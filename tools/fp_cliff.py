"""Times the order-dependent float folds on one huge group / partition:
the bit-exact one-lane replay (fp_parallel_min = never) against the parallel
form (the default from 2^20 rows), with the oracle's sequential C loop on a
10M-row sample beside them.

    python tools/fp_cliff.py [rows]      -> one JSON object on stdout

With --groups K and / or --partitions K (default 4) the same over K equal
segments instead: the grouped dbl average and stdev over K interleaved
groups, the running dbl SUM over K contiguous partitions, replay against
parallel.  --small-groups G times the grouped average and stdev over G
small groups (none reaches the threshold) at the default knob; --reps N
sets the timed repetitions.  A trailing "par" skips the replay legs.

--window {avg,stddev_samp,correlation} adds that window function over the
same partitions (peer groups of 16 rows) beside the running SUM, for --frame
{3,4,5} (default 3; the running SUM stays frame 3 / 4), with every timed
repetition listed ("samples_ms").
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
from oracle import pyoracle as ora  # noqa: E402


def timed(fn, reps):
    fn()
    gdk.sync()
    t = time.perf_counter()
    for _ in range(reps):
        out = fn()
    gdk.sync()
    return out, (time.perf_counter() - t) / reps * 1e3


def samples(fn, reps):
    """each of reps further calls on its own, in ms"""
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        gdk.sync()
        ms.append(round((time.perf_counter() - t) * 1e3, 3))
    return ms


def segments(n, ngroups, nparts, nsmall, par_only, reps, window=None, frame=3):
    """replay against parallel over several equal groups / partitions"""
    gdk.init(0)
    r = np.random.default_rng(5)
    x = r.standard_normal(n) * 100.0 + 50.0
    B = gdk.BAT.from_numpy(gdk.TYPE_dbl, x, sorted_=False, revsorted=False, key=False)
    ops = {}
    if ngroups or nsmall:
        k = ngroups or nsmall
        g = gdk.BAT.from_numpy(gdk.TYPE_oid, np.arange(n, dtype=np.uint64) % np.uint64(k), sorted_=False,
                               revsorted=False, key=False)
        e = gdk.BAT.dense(0, k)
        tag = "%d_groups" % k
        ops["groupavg_" + tag] = lambda: gdk.BATgroupavg(B, g, e, True)[0]
        ops["groupstdev_" + tag] = lambda: gdk.BATgroupstdev_population(B, g, e, True)
    if nparts:
        p = np.zeros(n, np.int8)
        p[::(n + nparts - 1) // nparts] = 1
        o = p.copy()
        o[::16] = 1                   # peer groups of 16 rows
        P, O = gdk.BAT.from_numpy(gdk.TYPE_bit, p), gdk.BAT.from_numpy(gdk.TYPE_bit, o)
        ops["running_sum_%d_partitions" % nparts] = lambda: gdk.GDKanalyticalsum(B, P, O, None, None, gdk.TYPE_dbl,
                                                                                 4 if frame == 4 else 3)
        wtag = "window_%s_frame%d_%d_partitions" % (window, frame, nparts)
        if window == "avg":
            ops[wtag] = lambda: gdk.GDKanalyticalavg(B, P, O, None, None, frame)
        elif window == "stddev_samp":
            ops[wtag] = lambda: gdk.GDKanalytical_stat(window, B, None, P, O, None, None, frame)
        elif window == "correlation":
            y = 0.5 * x + (r.standard_normal(n) * 100.0 + 50.0) * 0.3
            B2 = gdk.BAT.from_numpy(gdk.TYPE_dbl, y, sorted_=False, revsorted=False, key=False)
            ops[wtag] = lambda: gdk.GDKanalytical_stat(window, B, B2, P, O, None, None, frame)
    res = {"rows": n}
    for name, dev in ops.items():
        par, ms_par = timed(dev, reps)
        d = {"parallel_ms" if not nsmall else "ms": round(ms_par, 3)}
        if window:
            d["samples_ms"] = samples(dev, reps)
        if not par_only and not nsmall:
            prev = gdk.set_fp_parallel_min(None)
            try:
                seq, ms_seq = timed(dev, 1)
            finally:
                gdk.set_fp_parallel_min(prev)
            a, b = seq.to_numpy(), par.to_numpy()
            d["replay_ms"] = round(ms_seq, 3)
            d["max_abs_diff"] = float(np.nanmax(np.abs(a - b)))
            d["max_abs_value"] = float(np.nanmax(np.abs(a)))
        res[name] = d
        print(json.dumps({name: d}), file=sys.stderr, flush=True)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rows", nargs="?", type=int, default=100_000_000)
    ap.add_argument("par", nargs="?", choices=["par"])
    ap.add_argument("--groups", nargs="?", type=int, const=4, default=0)
    ap.add_argument("--partitions", nargs="?", type=int, const=4, default=0)
    ap.add_argument("--small-groups", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", choices=["avg", "stddev_samp", "correlation"])
    ap.add_argument("--frame", type=int, choices=[3, 4, 5], default=3)
    args = ap.parse_args()
    n = args.rows
    par_only = args.par == "par"     # profiling runs: no replay, no oracle
    if args.window and not args.partitions:
        args.partitions = 4
    if args.groups or args.partitions or args.small_groups:
        segments(n, 0 if args.small_groups else args.groups, args.partitions, args.small_groups, par_only, args.reps,
                 args.window, args.frame)
        return
    ns = min(n, 10_000_000)
    gdk.init(0)
    r = np.random.default_rng(5)
    x = r.standard_normal(n) * 100.0 + 50.0
    B = gdk.BAT.from_numpy(gdk.TYPE_dbl, x, sorted_=False, revsorted=False, key=False)
    OS = ora.Bat.from_array(ora.TYPE_dbl, x[:ns])
    g = gdk.BATconstant(gdk.TYPE_oid, 0, n)
    e = gdk.BAT.dense(0, 1)
    o = np.zeros(n, np.int8)
    o[::16] = 1                       # peer groups of 16 rows
    O = gdk.BAT.from_numpy(gdk.TYPE_bit, o)
    ops = {
        "stdev_population": (lambda: gdk.BATcalcvariance(B, False, stdev=True)[0],
                             lambda: ora.BATcalcstat("stdev", OS, None, False)[0]),
        "groupavg_one_group": (lambda: float(gdk.BATgroupavg(B, g, e, True)[0].to_numpy()[0]),
                               lambda: float(np.asarray(ora.BATgroupavg(
                                   OS, ora.Bat.from_array(ora.TYPE_oid, np.zeros(ns, np.uint64)),
                                   ora.Bat.dense(0, 1), True)[0].values())[0])),
        "running_sum_unpartitioned": (lambda: gdk.GDKanalyticalsum(B, None, O, None, None, gdk.TYPE_dbl, 3),
                                      lambda: ora.analyticalsum(OS, None, ora.Bat.from_array(ora.TYPE_bit, o[:ns]),
                                                                None, None, ora.TYPE_dbl, 3)),
    }
    res = {"rows": n, "oracle_sample_rows": ns}
    for name, (dev, orf) in ops.items():
        par, ms_par = timed(dev, 5)
        if par_only:
            res[name] = {"parallel_ms": round(ms_par, 3)}
            print(json.dumps({name: res[name]}), file=sys.stderr, flush=True)
            continue
        prev = gdk.set_fp_parallel_min(None)
        try:
            seq, ms_seq = timed(dev, 1)
        finally:
            gdk.set_fp_parallel_min(prev)
        t = time.perf_counter()
        orf()
        ms_ora = (time.perf_counter() - t) * 1e3 * n / ns
        d = {"replay_ms": round(ms_seq, 3), "parallel_ms": round(ms_par, 3),
             "oracle_ms_scaled": round(ms_ora, 1)}
        if isinstance(seq, float):
            d["replay"] = seq
            d["parallel"] = par
            d["diff_ulp"] = float(abs(seq - par) / np.spacing(abs(seq))) if seq == seq else None
        else:
            a, b = seq.to_numpy(), par.to_numpy()
            d["max_abs_diff"] = float(np.nanmax(np.abs(a - b)))
            d["max_abs_value"] = float(np.nanmax(np.abs(a)))
        res[name] = d
        print(json.dumps({name: d}), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
