"""The star route of the grouped MAL rewrite (monetdb_amd/mal.py,
fuse_star_groupsum): what it recognises and what it leaves alone and the
order of the calls (a stub binding, no GPU), an SSB-Q2-shaped plan -- a fact
predicate, a dimension predicate, a key through a second dimension, the sum of
a product -- against the oracle, rewritten and as written, and on the device
the rewritten plan through gdk.select_groupsum_star against the plan as
written, output by output."""
import numpy as np
import pytest

import test_mal_fuse_group_hash as MH
from monetdb_amd import mal


def P(res, left, col):
    return ((res,), "algebra.projection", (left, col))


FACT_PRED = [(("c1",), "algebra.select", ("qty", "s0", 2, 40, True, False, False))]
DIM_PRED = [P("t1", "c1", "ipart"), P("x1", "t1", "pbrand"),
            (("p1",), "algebra.thetaselect", ("x1", 7, "<")), P("c2", "p1", "c1")]
DIM_PRED_PATH = [(("x1",), "algebra.projectionpath", ("c1", "ipart", "pbrand")),
                 (("p1",), "algebra.thetaselect", ("x1", 7, "<")), P("c2", "p1", "c1")]
KEY_PATH = [(("ky",), "algebra.projectionpath", ("c2", "idate", "dyear"))]
KEY_TWO_STEPS = [P("ty", "c2", "idate"), P("ky", "ty", "dyear")]
REST = [P("pv", "c2", "price"), P("pd", "c2", "disc"), P("tw", "c2", "ipart"), P("pw", "tw", "pweight"),
        (("g", "e", "h"), "group.group", ("ky",)),
        (("f",), "batcalc.-:lng", (100, "pd")),
        (("m",), "batcalc.*:hge", ("pv", "f")),
        (("r1",), "aggr.subsum:hge", ("m", "g", "e")),
        (("r2",), "aggr.subsum:hge", ("pw", "g", "e")),
        (("n",), "aggr.subcount", ("ky", "g", "e")),
        P("kk", "e", "ky"), P("fr", "e", "c2")]
Q2 = FACT_PRED + DIM_PRED + KEY_PATH + REST
Q2_OTHER_FORMS = FACT_PRED + DIM_PRED_PATH + KEY_TWO_STEPS + REST
OUTS = ("r1", "r2", "n", "kk", "fr")
# one dimension column through two join indexes: GROUP BY the year of the order date and of the commit date
TWO_ROUTES = FACT_PRED + [
    (("ky",), "algebra.projectionpath", ("c1", "idate", "dyear")), P("t2", "c1", "idate2"), P("k2", "t2", "dyear"),
    P("pv", "c1", "price"),
    (("g1", "e1", "h1"), "group.group", ("ky",)), (("g", "e", "h"), "group.subgroup", ("k2", "g1")),
    (("r1",), "aggr.subsum:hge", ("pv", "g", "e")), (("n",), "aggr.subcount", ("ky", "g", "e")),
    P("kk", "e", "ky"), P("kc", "e", "k2"), P("fr", "e", "c1")]
TWO_OUTS = ("r1", "n", "kk", "kc", "fr")
# the first select on a column gathered for every row, no candidate-list variable before it
FIRST_GATHERED = [P("x0", "ipart", "pbrand"), (("c2",), "algebra.thetaselect", ("x0", 7, "<"))] + KEY_PATH + REST


def make_env(mod, n, seed=0):
    r = np.random.default_rng(seed)
    nparts, ndates = 1_000, 2_556
    h = {"qty": ("int", r.integers(0, 50, n).astype(np.int32)), "price": ("lng", r.integers(1, 1 << 40, n).astype(np.int64)),
         "disc": ("sht", r.integers(0, 11, n).astype(np.int16)),
         "ipart": ("oid", (r.integers(0, nparts, n) + 500).astype(np.uint64)),
         "idate": ("oid", r.integers(0, ndates, n).astype(np.uint64))}
    h["ipart"][1][r.random(n) < 0.02] = 1 << 63
    h["idate"][1][r.random(n) < 0.02] = 1 << 63
    h["idate2"] = ("oid", np.minimum(h["idate"][1] + r.integers(0, 400, n).astype(np.uint64), ndates - 1))
    h["price"][1][r.random(n) < 0.02] = -(1 << 63)
    mk = mod.BAT.from_numpy if hasattr(mod, "BAT") else mod.Bat.from_array
    env = {c: mk(getattr(mod, "TYPE_" + t), v) for c, (t, v) in h.items()}
    env["pbrand"] = mk(mod.TYPE_sht, r.integers(0, 40, nparts).astype(np.int16), hseqbase=500)
    env["pweight"] = mk(mod.TYPE_int, r.integers(-1000, 1000, nparts).astype(np.int32), hseqbase=500)
    env["dyear"] = mk(mod.TYPE_int, (1992 + np.arange(ndates) // 366).astype(np.int32))
    env["s0"] = (mod.BAT if hasattr(mod, "BAT") else mod.Bat).dense(100, n - 300)
    return env


def stub_binding(ora):
    """The oracle's operators plus fused entries that record the call and decline."""
    calls = []

    class Stub:
        def __getattr__(self, name):
            return getattr(ora, name)

        def select_groupsum(self, *a, **kw):
            calls.append("narrow")

        def select_groupsum_hash(self, *a, **kw):
            calls.append("hash")

        def select_groupsum_star(self, preds, keys, sums, vias, s=None, fused=True, fallback=True):
            assert fused and not fallback and s is not None
            # a route is a descriptor: every pair names its own, and the keys are among them
            assert len({id(d) for d, _ in vias}) == len(vias) and all(any(k is d for d, _ in vias) for k in keys)
            calls.append(("star", len(preds), len(keys), len(sums), len(vias)))

        def BATslice(self, b, lo, hi):
            assert lo == 0 and hi == b.count()
            calls.append("view")
            return ora.Bat.from_array(b.s.type, b.values(), hseqbase=b.s.hseqbase)

        def BATgroup(self, *a):
            if not calls or calls[-1] != "kept":
                calls.append("kept")
            return ora.BATgroup(*a)

    return Stub(), calls


def test_what_is_recognised():
    for plan in (Q2, Q2_OTHER_FORMS):
        rewritten = mal.fuse_star_groupsum(plan)
        assert [fn for _, fn, _ in rewritten] == ["mgdk.select_groupsum"]
        spec = rewritten[0][2][0]
        assert spec["vias"] == {"ipart->pbrand": ("pbrand", "ipart"), "idate->dyear": ("dyear", "idate"),
                                "ipart->pweight": ("pweight", "ipart")}
        assert [p[:2] for p in spec["preds"]] == [("algebra.select", "qty"), ("algebra.thetaselect", "ipart->pbrand")]
        assert spec["keys"] == ["idate->dyear"] and spec["s"] == "s0"
        assert spec["sums"] == [("price", ("-", 100, "disc")), ("ipart->pweight",)]
        assert spec["kept"] == plan
        # the plain grouped rewrite does not know a gathered column
        assert mal.fuse_select_groupsum(plan) == plan
    # an intermediate that something outside the fragment reads: left alone
    assert mal.fuse_star_groupsum(Q2 + [P("out", "t1", "pweight")]) == Q2 + [P("out", "t1", "pweight")]


def test_plans_without_gathers_are_rewritten_as_before():
    for plan in (MH.TWO_KEYS, MH.ONE_KEY, MH.K_ALONE):
        assert mal.fuse_star_groupsum(plan) == mal.fuse_select_groupsum(plan)
        assert "vias" not in mal.fuse_star_groupsum(plan)[0][2][0]


def test_first_select_on_a_gathered_column_is_left_as_written():
    assert mal.fuse_star_groupsum(FIRST_GATHERED) == FIRST_GATHERED


def test_order_of_calls(ora):
    env = make_env(ora, 1_003)
    want = MH.outputs(mal.run_plan(ora, Q2, env, fuse=False), OUTS)
    stub, calls = stub_binding(ora)
    assert MH.outputs(mal.run_plan(stub, Q2, env, star=True), OUTS) == want
    assert calls == [("star", 2, 1, 2, 3), "kept"]
    # without the star rewrite the plan runs as written
    stub, calls = stub_binding(ora)
    assert MH.outputs(mal.run_plan(stub, Q2, env, star=False), OUTS) == want
    assert calls == ["kept"]
    # a plan without gathers takes the routes it took, star or not
    n = 1_003
    h, types = MH.make_cols(n, 1, 4, 3, "sht")
    henv = MH.env_of(ora, h, types, n)
    for star in (False, True):
        stub, calls = stub_binding(ora)
        mal.run_plan(stub, MH.K_ALONE, henv, hashed=True, star=star)
        assert calls == ["hash", "kept"]
    # a join index that is no oid column: the kept instructions, the star entry is not asked
    stub, calls = stub_binding(ora)
    bad = dict(env, idate=ora.Bat.from_array(ora.TYPE_lng, np.zeros(1_003, np.int64)))
    with pytest.raises(Exception):
        mal.run_plan(stub, Q2, bad, star=True)
    assert calls == []


def test_two_routes_to_one_column(ora):
    """The second route to a dimension column gets a descriptor of its own (a view), on the stub and in the
    spec; the plan's results are those of the plan as written."""
    rewritten = mal.fuse_star_groupsum(TWO_ROUTES)
    assert [fn for _, fn, _ in rewritten] == ["mgdk.select_groupsum"]
    spec = rewritten[0][2][0]
    assert spec["vias"] == {"idate->dyear": ("dyear", "idate"), "idate2->dyear": ("dyear", "idate2")}
    assert spec["keys"] == ["idate->dyear", "idate2->dyear"]
    env = make_env(ora, 5_003, 2)
    want = MH.outputs(mal.run_plan(ora, TWO_ROUTES, env, fuse=False), TWO_OUTS)
    assert len(want["n"]) > 8 and want["kk"] != want["kc"]
    stub, calls = stub_binding(ora)
    assert MH.outputs(mal.run_plan(stub, TWO_ROUTES, env, star=True), TWO_OUTS) == want
    assert calls == ["view", ("star", 1, 2, 1, 2), "kept"]


def test_q2_shape_against_the_oracle(ora):
    env = make_env(ora, 20_011, 3)
    for plan in (Q2, Q2_OTHER_FORMS):
        plain = MH.outputs(mal.run_plan(ora, plan, env, fuse=False), OUTS)
        assert len(plain["n"]) == 8 and -(1 << 31) in plain["kk"]          # seven years and the nil oids' nil key
        assert MH.outputs(mal.run_plan(ora, mal.fuse_star_groupsum(plan), env), OUTS) == plain
        assert MH.outputs(mal.run_plan(ora, plan, env, star=True), OUTS) == plain


@pytest.mark.gpu
def test_q2_shape_on_the_device(gdk, ora):
    """The rewritten plan on the product equals the plan as written on the product and on the
    oracle, output by output, and it is the star fused operator that ran it, once."""
    n = 70_001
    ge, oe = make_env(gdk, n, 3), make_env(ora, n, 3)
    gdk.prof_enable(True)
    try:
        for plan, outs in ((Q2, OUTS), (Q2_OTHER_FORMS, OUTS), (TWO_ROUTES, TWO_OUTS)):
            want = MH.outputs(mal.run_plan(ora, plan, oe, fuse=False), outs)
            before = gdk.prof_get("select_groupsum_star_fused")[1]
            plain = MH.outputs(mal.run_plan(gdk, plan, ge, fuse=False), outs)
            assert gdk.prof_get("select_groupsum_star_fused")[1] == before
            fused = MH.outputs(mal.run_plan(gdk, plan, ge, star=True), outs)
            assert gdk.prof_get("select_groupsum_star_fused")[1] == before + 1
            for k in outs:
                assert fused[k] == plain[k] == want[k], k
    finally:
        gdk.prof_enable(False)
