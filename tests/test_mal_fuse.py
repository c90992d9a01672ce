"""The MAL plan runner and the select-cascade + SUM rewrite (monetdb_amd.mal):
fuse_select_sum on plan shapes, run_plan against the oracle (no GPU) and
against the product, where the rewritten plan takes the fused operator."""
import numpy as np
import pytest

from monetdb_amd import mal


def q6_plan(d0, d1):
    """the seven instructions of TPC-H Q6 (per slice)."""
    return [
        (("c1",), "algebra.select", ("shipdate", d0, d1, True, False, False)),
        (("c2",), "algebra.select", ("discount", "c1", 5, 7, True, True, False)),
        (("c3",), "algebra.thetaselect", ("quantity", "c2", 2400, "<")),
        (("p1",), "algebra.projection", ("c3", "extendedprice")),
        (("p2",), "algebra.projection", ("c3", "discount")),
        (("m",), "batcalc.*:hge", ("p1", "p2")),
        (("r",), "aggr.sum:hge", ("m",)),
    ]


COUNT_PLAN = [
    (("c1",), "algebra.thetaselect", ("a", 3, "!=")),
    (("c2",), "algebra.select", ("b", "c1", 1, 9, True, True, False)),
    (("n",), "aggr.count", ("c2",)),
]

TWO_SUMS_PLAN = [
    (("c1",), "algebra.select", ("a", "s0", 2, 40, True, False, False)),
    (("c2",), "algebra.thetaselect", ("b", "c1", 5, "!=")),
    (("pa",), "algebra.projection", ("c2", "a")),
    (("pb",), "algebra.projection", ("c2", "b")),
    (("pv",), "algebra.projection", ("c2", "v")),
    (("m",), "batcalc.*:hge", ("pv", "pb")),
    (("r1",), "aggr.sum:hge", ("m",)),
    (("r2",), "aggr.sum:hge", ("pa",)),
    (("n",), "aggr.count", ("c2",)),
]


def fn_names(plan):
    return [ins[1] for ins in plan]


def test_fuse_q6_plan():
    plan = q6_plan(100, 200)
    fused = mal.fuse_select_sum(plan)
    assert fn_names(fused) == ["mgdk.select_sum"]
    res, _, (spec,) = fused[0]
    assert res == ("r",)
    assert spec["s"] is None
    assert [(fn, col) for fn, col, _ in spec["preds"]] == [
        ("algebra.select", "shipdate"), ("algebra.select", "discount"), ("algebra.thetaselect", "quantity")]
    assert spec["preds"][0][2] == (100, 200, True, False, False)
    assert spec["preds"][2][2] == (2400, "<")
    assert spec["sums"] == [("extendedprice", "discount")]
    assert spec["kept"] == plan
    assert plan == q6_plan(100, 200)          # the input is left as it was


def test_fuse_count_only_plan():
    fused = mal.fuse_select_sum(COUNT_PLAN)
    assert fn_names(fused) == ["mgdk.select_sum"]
    res, _, (spec,) = fused[0]
    assert res == ("n",) and spec["sums"] == [] and len(spec["preds"]) == 2
    assert spec["kept"] == COUNT_PLAN


def test_fuse_two_sums_and_count_from_a_candidate():
    fused = mal.fuse_select_sum(TWO_SUMS_PLAN)
    assert fn_names(fused) == ["mgdk.select_sum"]
    res, _, (spec,) = fused[0]
    assert res == ("r1", "r2", "n")
    assert spec["s"] == "s0"
    assert spec["sums"] == [("v", "b"), ("a", None)]


def test_fuse_keeps_surrounding_instructions():
    extra = [(("z",), "algebra.projection", ("s0", "v"))]
    tail = [(("k",), "aggr.count", ("z",))]
    fused = mal.fuse_select_sum(extra + TWO_SUMS_PLAN + tail)
    assert fn_names(fused) == ["algebra.projection", "mgdk.select_sum", "aggr.count"]


def replace(plan, i, ins):
    return plan[:i] + [ins] + plan[i + 1:]


@pytest.mark.parametrize("why", ["cand_second_use", "proj_second_use", "product_not_hge", "cand_not_from_chain",
                                 "proj_other_cand", "sum_not_hge", "five_selects"])
def test_fuse_leaves_plan_unchanged(why):
    plan = q6_plan(100, 200)
    if why == "cand_second_use":        # c2 also feeds a projection outside the chain
        plan = plan + [(("x",), "algebra.projection", ("c2", "quantity"))]
    elif why == "proj_second_use":      # p2 is needed by something that is not part of the fragment
        plan = plan + [(("x",), "batcalc.+:hge", ("p2", "p2"))]
    elif why == "product_not_hge":
        plan = replace(plan, 5, (("m",), "batcalc.*:lng", ("p1", "p2")))
    elif why == "cand_not_from_chain":  # c2's candidate list is a projection's result
        plan = [(("c1",), "algebra.projection", ("s0", "oids"))] + plan[1:]
    elif why == "proj_other_cand":      # one operand is projected through c2, not c3
        plan = replace(plan, 4, (("p2",), "algebra.projection", ("c2", "discount")))
    elif why == "sum_not_hge":
        plan = replace(plan, 6, (("r",), "aggr.sum:lng", ("m",)))
    elif why == "five_selects":
        more = [(("c4",), "algebra.thetaselect", ("quantity", "c3", 1, ">")),
                (("c5",), "algebra.thetaselect", ("quantity", "c4", 2, ">")),
                (("p1",), "algebra.projection", ("c5", "extendedprice")),
                (("p2",), "algebra.projection", ("c5", "discount"))]
        plan = plan[:3] + more + plan[5:]
    assert mal.fuse_select_sum(plan) == plan


def ora_env(ora, host):
    tp = {"shipdate": ora.TYPE_date}
    return {k: ora.Bat.from_array(tp.get(k, ora.TYPE_lng), host[k])
            for k in ("shipdate", "discount", "quantity", "extendedprice")}


def test_run_plan_oracle_q6(ora):
    n = 100_003
    host = ora.tpch_lineitem(5, 0, n, 20_000)
    plan = q6_plan(ora.mkdate(1994, 1, 1), ora.mkdate(1995, 1, 1))
    want = ora.q6(host, 1)
    env = ora_env(ora, host)
    assert mal.run_plan(ora, plan, env, fuse=False)["r"] == want
    # the oracle has no select_sum: the fused instruction runs what it kept
    assert mal.run_plan(ora, mal.fuse_select_sum(plan), env)["r"] == want
    assert mal.run_plan(ora, plan, env, fuse=True)["r"] == want


def small_cols(n, seed):
    r = np.random.default_rng(seed)
    a = r.integers(0, 50, n).astype(np.int32)
    b = r.integers(0, 12, n).astype(np.int16)
    v = r.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    a[r.random(n) < 0.02] = np.iinfo(np.int32).min
    b[r.random(n) < 0.02] = np.iinfo(np.int16).min
    v[r.random(n) < 0.02] = np.iinfo(np.int64).min
    return {"a": a, "b": b, "v": v}


def test_run_plan_oracle_other_plans(ora):
    n = 5_003
    h = small_cols(n, 3)
    env = {"a": ora.Bat.from_array(ora.TYPE_int, h["a"]), "b": ora.Bat.from_array(ora.TYPE_sht, h["b"]),
           "v": ora.Bat.from_array(ora.TYPE_lng, h["v"]), "s0": ora.Bat.dense(100, n - 300)}
    got = mal.run_plan(ora, TWO_SUMS_PLAN, env, fuse=False)
    lo, hi = 100, n - 200
    a, b, v = (h[k][lo:hi].astype(object) for k in "abv")
    nil_a, nil_b, nil_v = -(1 << 31), -(1 << 15), -(1 << 63)
    keep = [(x != nil_a and 2 <= x < 40) and (y != nil_b and y != 5) for x, y in zip(a, b)]
    assert got["n"] == sum(keep)
    assert got["r1"] == sum(int(z) * int(y) for k, y, z in zip(keep, b, v) if k and z != nil_v)
    assert got["r2"] == sum(int(x) for k, x in zip(keep, a) if k)
    fused = mal.run_plan(ora, mal.fuse_select_sum(TWO_SUMS_PLAN), env)
    assert (fused["r1"], fused["r2"], fused["n"]) == (got["r1"], got["r2"], got["n"])
    cnt = mal.run_plan(ora, COUNT_PLAN, env, fuse=False)["n"]
    assert cnt == sum(1 for x, y in zip(h["a"], h["b"]) if x != nil_a and x != 3 and y != nil_b and 1 <= y <= 9)
    assert mal.run_plan(ora, mal.fuse_select_sum(COUNT_PLAN), env)["n"] == cnt


@pytest.mark.gpu
def test_fused_plans_on_the_device(gdk, ora):
    """The rewritten plan on the product equals the plan as written on the
    product and on the oracle, and it is the fused operator that ran it."""
    n = 100_003
    host = ora.tpch_lineitem(5, 0, n, 20_000)
    cols = gdk.tpch_lineitem(5, 0, n, 20_000)
    q6 = q6_plan(ora.mkdate(1994, 1, 1), ora.mkdate(1995, 1, 1))
    h = small_cols(70_001, 4)
    m = len(h["a"])
    genv = {"a": gdk.BAT.from_numpy(gdk.TYPE_int, h["a"]), "b": gdk.BAT.from_numpy(gdk.TYPE_sht, h["b"]),
            "v": gdk.BAT.from_numpy(gdk.TYPE_lng, h["v"]), "s0": gdk.BAT.dense(100, m - 300)}
    oenv = {"a": ora.Bat.from_array(ora.TYPE_int, h["a"]), "b": ora.Bat.from_array(ora.TYPE_sht, h["b"]),
            "v": ora.Bat.from_array(ora.TYPE_lng, h["v"]), "s0": ora.Bat.dense(100, m - 300)}
    cases = [(q6, {k: cols[k] for k in ("shipdate", "discount", "quantity", "extendedprice")}, ora_env(ora, host),
              ("r",)),
             (COUNT_PLAN, genv, oenv, ("n",)),           # int and sht predicates with a !=
             (TWO_SUMS_PLAN, genv, oenv, ("r1", "r2", "n"))]   # starts from a dense candidate
    gdk.prof_enable(True)
    try:
        for plan, ge, oe, outs in cases:
            want = mal.run_plan(ora, plan, oe, fuse=False)
            before = gdk.prof_get("select_sum_fused")[1]
            plain = mal.run_plan(gdk, plan, ge, fuse=False)
            assert gdk.prof_get("select_sum_fused")[1] == before
            fused = mal.run_plan(gdk, mal.fuse_select_sum(plan), ge)
            assert gdk.prof_get("select_sum_fused")[1] == before + 1
            for k in outs:
                assert fused[k] == plain[k] == want[k], k
        assert mal.run_plan(gdk, q6, cases[0][1])["r"] == ora.q6(host, 1)          # fused by default
    finally:
        gdk.prof_enable(False)
