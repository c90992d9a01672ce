"""The MAL rewrite of the grouped select cascade (monetdb_amd/mal.py):
fuse_select_groupsum on plan shapes, run_plan of grouped plans against the
oracle (no GPU) and, on the device, the rewritten plan against the plan as
written, output by output."""
import copy

import numpy as np
import pytest

from monetdb_amd import mal


def P(res, col, left="c"):
    return ((res,), "algebra.projection", (left, col))


def q1_plan(dmax):
    """TPC-H Q1 as the SQL front end emits it per slice."""
    return [
        (("c",), "algebra.thetaselect", ("shipdate", dmax, "<=")),
        P("prf", "returnflag"), P("pls", "linestatus"), P("pq", "quantity"), P("pp", "extendedprice"),
        P("pd", "discount"), P("pt", "tax"),
        (("g1", "e1", "h1"), "group.group", ("prf",)),
        (("g", "e", "h"), "group.subgroup", ("pls", "g1")),
        (("omd",), "batcalc.-:lng", (100, "pd")),
        (("dp",), "batcalc.*:hge", ("pp", "omd")),
        (("opt",), "batcalc.+:lng", (100, "pt")),
        (("ch",), "batcalc.*:hge", ("dp", "opt")),
        (("s1",), "aggr.subsum:hge", ("pq", "g", "e")),
        (("s2",), "aggr.subsum:hge", ("pp", "g", "e")),
        (("s3",), "aggr.subsum:hge", ("dp", "g", "e")),
        (("s4",), "aggr.subsum:hge", ("ch", "g", "e")),
        (("s5",), "aggr.subsum:hge", ("pd", "g", "e")),
        (("cn",), "aggr.subcount", ("pq", "g", "e")),
        (("a1", "r1", "n1"), "aggr.subavg", ("pq", "g", "e")),
        (("a2", "r2", "n2"), "aggr.subavg", ("pp", "g", "e")),
        (("a3", "r3", "n3"), "aggr.subavg", ("pd", "g", "e")),
        P("krf", "prf", "e"), P("kls", "pls", "e"),
    ]


Q1_OUTS = ("s1", "s2", "s3", "s4", "s5", "cn", "a1", "r1", "n1", "a2", "r2", "n2", "a3", "r3", "n3", "krf", "kls")

# two keys from a dense candidate list, a range and a theta select, an affine
# factor of a sht column, a group whose every v is nil (k == 3)
SMALL_PLAN = [
    (("c1",), "algebra.select", ("a", "s0", 2, 40, True, False, False)),
    (("c2",), "algebra.thetaselect", ("b", "c1", 5, "!=")),
    P("pk", "k", "c2"), P("pj", "j", "c2"), P("pv", "v", "c2"), P("pb", "b", "c2"),
    (("g1", "e1", "h1"), "group.group", ("pk",)),
    (("g", "e", "h"), "group.subgroup", ("pj", "g1")),
    (("f",), "batcalc.+:lng", (7, "pb")),
    (("m",), "batcalc.*:hge", ("pv", "f")),
    (("r1",), "aggr.subsum:hge", ("m", "g", "e")),
    (("r2",), "aggr.subsum:hge", ("pv", "g", "e")),
    (("n",), "aggr.subcount", ("pk", "g", "e")),
    (("av", "rm", "nn"), "aggr.subavg", ("pv", "g", "e")),
    P("kk", "pk", "e"), P("kj", "pj", "e"), P("fr", "c2", "e"),
]
SMALL_OUTS = ("r1", "r2", "n", "av", "rm", "nn", "kk", "kj", "fr")


def fn_names(plan):
    return [fn.partition(":")[0] for _, fn, _ in plan]


def test_rewrite_q1():
    plan = q1_plan(10471)
    before = copy.deepcopy(plan)
    fused = mal.fuse_select_groupsum(plan)
    assert plan == before                                   # the input is left alone
    assert fn_names(fused) == ["mgdk.select_groupsum"]
    res, _, (spec,) = fused[0]
    assert res == Q1_OUTS
    assert spec["kept"] == plan
    assert spec["s"] is None and spec["preds"] == [("algebra.thetaselect", "shipdate", (10471, "<="))]
    assert spec["keys"] == ["returnflag", "linestatus"]
    assert spec["sums"] == [("quantity",), ("extendedprice",), ("extendedprice", ("-", 100, "discount")),
                            ("extendedprice", ("-", 100, "discount"), ("+", 100, "tax")), ("discount",)]
    assert spec["outs"] == [("sum", "s1", 0), ("sum", "s2", 1), ("sum", "s3", 2), ("sum", "s4", 3), ("sum", "s5", 4),
                            ("count", "cn"), ("avg", ("a1", "r1", "n1"), 0, "quantity"),
                            ("avg", ("a2", "r2", "n2"), 1, "extendedprice"), ("avg", ("a3", "r3", "n3"), 4, "discount"),
                            ("proj", "krf", "returnflag"), ("proj", "kls", "linestatus")]
    assert mal.fuse_select_groupsum(fused) == fused         # already rewritten: left as it is


def test_rewrite_small_plan_and_surroundings():
    fused = mal.fuse_select_groupsum(SMALL_PLAN)
    assert fn_names(fused) == ["mgdk.select_groupsum"]
    spec = fused[0][2][0]
    assert spec["s"] == "s0" and len(spec["preds"]) == 2 and spec["keys"] == ["k", "j"]
    assert spec["sums"] == [("v", ("+", 7, "b")), ("v",)]
    assert ("first", "fr") in spec["outs"]
    # instructions around the fragment stay, a sixth sum still fits
    extra = [P("pa", "a", "c2"), (("r6",), "aggr.subsum:hge", ("pa", "g", "e"))]
    tail = [(("srt",), "algebra.projection", ("kk", "a"))]
    plan = SMALL_PLAN[:6] + [extra[0]] + SMALL_PLAN[6:] + [extra[1]] + tail
    fused = mal.fuse_select_groupsum(plan)
    assert fn_names(fused) == ["mgdk.select_groupsum", "algebra.projection"]


def swap(plan, res, ins):
    return [ins if r[0] == res else (r, fn, a) for r, fn, a in plan]


@pytest.mark.parametrize("why", ["g_used_outside", "e_not_projected", "product_into_lng", "affine_into_int",
                                 "three_keys", "seven_sums", "other_candidate_list", "h_used", "cand_used_outside"])
def test_unchanged(why):
    plan = q1_plan(10471)
    if why == "g_used_outside":
        plan.append(P("z", "quantity", "g"))
    elif why == "e_not_projected":
        plan.append((("z",), "aggr.count", ("e",)))
    elif why == "product_into_lng":
        plan = swap(plan, "dp", (("dp",), "batcalc.*:lng", ("pp", "omd")))
    elif why == "affine_into_int":
        plan = swap(plan, "omd", (("omd",), "batcalc.-:int", (100, "pd")))
    elif why == "three_keys":
        plan = [(r, fn, tuple("g3" if x == "g" else "e3" if x == "e" else x for x in a)) if fn.startswith("aggr.")
                or (fn == "algebra.projection" and a[0] == "e") else (r, fn, a) for r, fn, a in plan]
        plan.insert(9, (("g3", "e3", "h3"), "group.subgroup", ("pq", "g")))
    elif why == "seven_sums":
        plan += [(("x6",), "aggr.subsum:hge", ("pt", "g", "e")), (("qt",), "batcalc.*:hge", ("pq", "pt")),
                 (("x7",), "aggr.subsum:hge", ("qt", "g", "e"))]
    elif why == "other_candidate_list":
        plan += [(("c9",), "algebra.thetaselect", ("shipdate", 9000, ">")), P("pz", "tax", "c9"),
                 (("x6",), "aggr.subsum:hge", ("pz", "g", "e"))]
    elif why == "h_used":
        plan.append((("z",), "aggr.count", ("h",)))
    elif why == "cand_used_outside":
        plan.append((("z",), "aggr.count", ("c",)))
    assert mal.fuse_select_groupsum(plan) == plan


def q1_env(mod, host, cols=None):
    """Oracle: the flag columns as the bytes of their offsets (GRP_small_values groups them so)."""
    if cols is not None:
        return dict(cols)
    tp = {"shipdate": mod.TYPE_date, "returnflag": mod.TYPE_bte, "linestatus": mod.TYPE_bte}
    return {k: mod.Bat.from_array(tp.get(k, mod.TYPE_lng), host[k].view(np.int8) if k in ("returnflag", "linestatus")
                                  else host[k]) for k in host}


def outputs(env, names):
    return {k: [int(x) & 0xff if k.startswith("k") else int(x) for x in env[k].values()] for k in names}


def q1_rows(out):
    rows = []
    for i in range(len(out["cn"])):
        rows.append(dict(returnflag=out["krf"][i], linestatus=out["kls"][i], sum_qty=out["s1"][i],
                         sum_base_price=out["s2"][i], sum_disc_price=out["s3"][i], sum_charge=out["s4"][i],
                         avg_qty=out["a1"][i], avg_price=out["a2"][i], avg_disc=out["a3"][i], rem_qty=out["r1"][i],
                         rem_price=out["r2"][i], rem_disc=out["r3"][i], count_order=out["cn"][i]))
    return sorted(rows, key=lambda r: (r["returnflag"], r["linestatus"]))


def test_run_plan_oracle_q1(ora):
    n = 100_003
    host = ora.tpch_lineitem(5, 0, n, 20_000)
    plan = q1_plan(ora.mkdate(1998, 9, 2))
    want = sorted(ora.q1(host, 1), key=lambda r: (r["returnflag"], r["linestatus"]))
    env = q1_env(ora, host)
    plain = outputs(mal.run_plan(ora, plan, env, fuse=False), Q1_OUTS)
    assert q1_rows(plain) == want and len(want) >= 3
    assert plain["n1"] == plain["n2"] == plain["n3"] == plain["cn"]
    # the oracle has no select_groupsum: the fused instruction runs what it kept
    assert outputs(mal.run_plan(ora, mal.fuse_select_groupsum(plan), env), Q1_OUTS) == plain
    assert outputs(mal.run_plan(ora, plan, env, fuse=True), Q1_OUTS) == plain


def small_cols(n, seed):
    r = np.random.default_rng(seed)
    h = {"a": r.integers(0, 50, n).astype(np.int32), "b": r.integers(0, 12, n).astype(np.int16),
         "v": r.integers(-(1 << 40), 1 << 40, n).astype(np.int64), "k": r.integers(1, 4, n).astype(np.int8),
         "j": r.integers(0, 2, n).astype(np.int8)}
    for c in "abv":
        h[c][r.random(n) < 0.02] = np.iinfo(h[c].dtype).min
    h["v"][h["k"] == 3] = np.iinfo(np.int64).min          # a group without a non-nil v
    return h


SMALL_TYPES = {"a": "int", "b": "sht", "v": "lng", "k": "bte", "j": "bte"}


def test_run_plan_oracle_small_plan(ora):
    n = 5_003
    h = small_cols(n, 3)
    env = {c: ora.Bat.from_array(getattr(ora, "TYPE_" + t), h[c]) for c, t in SMALL_TYPES.items()}
    env["s0"] = ora.Bat.dense(100, n - 300)
    got = outputs(mal.run_plan(ora, SMALL_PLAN, env, fuse=False), SMALL_OUTS)
    nil = {c: int(np.iinfo(h[c].dtype).min) for c in h}
    groups, order = {}, []
    for i in range(100, n - 200):
        a, b, v = int(h["a"][i]), int(h["b"][i]), int(h["v"][i])
        if a == nil["a"] or not 2 <= a < 40 or b == nil["b"] or b == 5:
            continue
        key = (int(h["k"][i]), int(h["j"][i]))
        if key not in groups:
            groups[key] = dict(first=i, n=0, r1=0, r2=0, nn=0)
            order.append(key)
        g = groups[key]
        g["n"] += 1
        if v != nil["v"]:
            g["r1"] += v * (7 + b)
            g["r2"] += v
            g["nn"] += 1
    assert len(order) == 6
    assert got["kk"] == [k[0] for k in order] and got["kj"] == [k[1] for k in order]
    assert got["fr"] == [groups[k]["first"] for k in order] and got["n"] == [groups[k]["n"] for k in order]
    hnil = -(1 << 127)
    assert got["r1"] == [groups[k]["r1"] if groups[k]["nn"] else hnil for k in order]
    assert got["r2"] == [groups[k]["r2"] if groups[k]["nn"] else hnil for k in order]
    assert got["nn"] == [groups[k]["nn"] for k in order]
    for k, av, rm in zip(order, got["av"], got["rm"]):
        g = groups[k]
        if g["nn"] == 0:
            assert (av, rm) == (nil["v"], 0)
        else:
            assert av * g["nn"] + rm == g["r2"] and abs(2 * rm) <= g["nn"]
    assert outputs(mal.run_plan(ora, mal.fuse_select_groupsum(SMALL_PLAN), env), SMALL_OUTS) == got


@pytest.mark.gpu
def test_fused_plans_on_the_device(gdk, ora):
    """The rewritten plan on the product equals the plan as written on the
    product and on the oracle, output by output, and it is the fused operator
    that ran it -- once per rewritten plan."""
    n = 100_003
    host = ora.tpch_lineitem(5, 0, n, 20_000)
    cols = gdk.tpch_lineitem(5, 0, n, 20_000)
    q1 = q1_plan(ora.mkdate(1998, 9, 2))
    m = 70_001
    h = small_cols(m, 4)
    genv = {c: gdk.BAT.from_numpy(getattr(gdk, "TYPE_" + t), h[c]) for c, t in SMALL_TYPES.items()}
    oenv = {c: ora.Bat.from_array(getattr(ora, "TYPE_" + t), h[c]) for c, t in SMALL_TYPES.items()}
    genv["s0"], oenv["s0"] = gdk.BAT.dense(100, m - 300), ora.Bat.dense(100, m - 300)
    cases = [(q1, q1_env(gdk, None, cols), q1_env(ora, host), Q1_OUTS), (SMALL_PLAN, genv, oenv, SMALL_OUTS)]
    gdk.prof_enable(True)
    try:
        for plan, ge, oe, outs in cases:
            want = outputs(mal.run_plan(ora, plan, oe, fuse=False), outs)
            before = gdk.prof_get("select_groupsum_fused")[1]
            plain = outputs(mal.run_plan(gdk, plan, ge, fuse=False), outs)
            assert gdk.prof_get("select_groupsum_fused")[1] == before
            rewritten = mal.fuse_select_groupsum(plan)
            assert fn_names(rewritten) == ["mgdk.select_groupsum"]
            fused = outputs(mal.run_plan(gdk, rewritten, ge), outs)
            assert gdk.prof_get("select_groupsum_fused")[1] == before + 1
            for k in outs:
                assert fused[k] == plain[k] == want[k], k
        assert 0 in want["nn"] and len(want["n"]) == 6       # the small plan's all-nil group went through subavg
    finally:
        gdk.prof_enable(False)
