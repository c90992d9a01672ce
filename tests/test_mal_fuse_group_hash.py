"""The hashed route of the grouped MAL rewrite (monetdb_amd/mal.py): which
fused operator a mgdk.select_groupsum tries and in what order (a stub binding,
no GPU), grouped plans on wider keys against the oracle, and on the device the
rewritten plans through gdk.select_groupsum_hash against the plans as written,
output by output."""
import numpy as np
import pytest

from monetdb_amd import mal


def P(res, col, left="c2"):
    return ((res,), "algebra.projection", (left, col))


HEAD = [
    (("c1",), "algebra.select", ("a", "s0", 2, 40, True, False, False)),
    (("c2",), "algebra.thetaselect", ("b", "c1", 5, "!=")),
    P("pk", "k"), P("pj", "j"), P("pv", "v"), P("pb", "b"),
]
TAIL = [
    (("f",), "batcalc.+:lng", (7, "pb")),
    (("m",), "batcalc.*:hge", ("pv", "f")),
    (("r1",), "aggr.subsum:hge", ("m", "g", "e")),
    (("r2",), "aggr.subsum:hge", ("pv", "g", "e")),
    (("n",), "aggr.subcount", ("pk", "g", "e")),
    (("av", "rm", "nn"), "aggr.subavg", ("pv", "g", "e")),
    P("kk", "pk", "e"), P("fr", "c2", "e"),
]
# GROUP BY (k, j) and GROUP BY j alone
TWO_KEYS = HEAD + [(("g1", "e1", "h1"), "group.group", ("pk",)), (("g", "e", "h"), "group.subgroup", ("pj", "g1"))] \
    + TAIL + [P("kj", "pj", "e")]
ONE_KEY = [i for i in HEAD if i[0] != ("pk",)] + [(("g", "e", "h"), "group.group", ("pj",))] \
    + [i for i in TAIL if i[0] not in (("n",), ("kk",))] + [(("n",), "aggr.subcount", ("pj", "g", "e")), P("kj", "pj", "e")]
# GROUP BY k alone
K_ALONE = [i for i in HEAD if i[0] != ("pj",)] + [(("g", "e", "h"), "group.group", ("pk",))] + TAIL
TWO_OUTS = ("r1", "r2", "n", "av", "rm", "nn", "kk", "kj", "fr")
ONE_OUTS = ("r1", "r2", "n", "av", "rm", "nn", "kj", "fr")
K_OUTS = ("r1", "r2", "n", "av", "rm", "nn", "kk", "fr")


def make_cols(n, seed, nk, nj, ktype="sht"):
    r = np.random.default_rng(seed)
    kdt = {"sht": np.int16, "bte": np.int8}[ktype]
    h = {"a": r.integers(0, 50, n).astype(np.int32), "b": r.integers(0, 12, n).astype(np.int16),
         "v": r.integers(-(1 << 40), 1 << 40, n).astype(np.int64),
         "k": (r.integers(0, nk, n) * (3 if ktype == "bte" else 1_000) - 5).astype(kdt),
         "j": (1990 + r.integers(0, nj, n)).astype(np.int32)}
    for c in "abv":
        h[c][r.random(n) < 0.02] = np.iinfo(h[c].dtype).min
    h["k"][r.random(n) < 0.02] = np.iinfo(kdt).min           # a nil key is a key
    h["v"][h["j"] == 1991] = np.iinfo(np.int64).min          # groups without a non-nil v
    return h, {"a": "int", "b": "sht", "v": "lng", "k": ktype, "j": "int"}


def env_of(mod, h, types, n):
    mk = mod.BAT.from_numpy if hasattr(mod, "BAT") else mod.Bat.from_array
    env = {c: mk(getattr(mod, "TYPE_" + t), h[c]) for c, t in types.items()}
    env["s0"] = (mod.BAT if hasattr(mod, "BAT") else mod.Bat).dense(100, n - 300)
    return env


def outputs(env, names):
    return {k: [int(x) for x in env[k].values()] for k in names}


def stub_binding(ora, with_hash):
    """The oracle's operators plus fused entries that record the call and decline."""
    calls = []

    class Stub:
        def __getattr__(self, name):
            return getattr(ora, name)

        def select_groupsum(self, preds, keys, sums, s=None, fused=True, fallback=True):
            assert fused and not fallback
            calls.append("narrow")

        def BATgroup(self, *a):
            if not calls or calls[-1] != "kept":
                calls.append("kept")
            return ora.BATgroup(*a)

    if with_hash:
        def select_groupsum_hash(self, preds, keys, sums, s=None, fused=True, fallback=True):
            assert fused and not fallback
            calls.append("hash")
        Stub.select_groupsum_hash = select_groupsum_hash
    return Stub(), calls


def test_route_order(ora):
    n = 1_003
    for ktype, plan, outs, narrow_first in (("bte", K_ALONE, K_OUTS, True), ("bte", TWO_KEYS, TWO_OUTS, False),
                                            ("sht", K_ALONE, K_OUTS, False), ("sht", ONE_KEY, ONE_OUTS, False)):
        h, types = make_cols(n, 1, 4, 3, ktype)
        env = env_of(ora, h, types, n)
        want = outputs(mal.run_plan(ora, plan, env, fuse=False), outs)
        rewritten = mal.fuse_select_groupsum(plan)
        assert [fn for _, fn, _ in rewritten] == ["mgdk.select_groupsum"]
        first = ["narrow"] if narrow_first else []
        for with_hash, hashed, order in ((True, True, first + ["hash", "kept"]), (True, False, first + ["kept"]),
                                         (False, True, first + ["kept"])):
            stub, calls = stub_binding(ora, with_hash)
            got = outputs(mal.run_plan(stub, rewritten, env, hashed=hashed), outs)
            assert calls == order, (ktype, with_hash, hashed)
            assert got == want
    # the oracle itself has neither entry: the kept instructions
    assert outputs(mal.run_plan(ora, rewritten, env, hashed=True), outs) == want


def test_run_plan_oracle_wider_keys(ora):
    n = 5_003
    h, types = make_cols(n, 3, 8, 5)
    env = env_of(ora, h, types, n)
    for plan, outs, ng in ((TWO_KEYS, TWO_OUTS, 45), (ONE_KEY, ONE_OUTS, 5)):
        plain = outputs(mal.run_plan(ora, plan, env, fuse=False), outs)
        assert len(plain["n"]) == ng and 0 in plain["nn"]
        assert outputs(mal.run_plan(ora, mal.fuse_select_groupsum(plan), env, hashed=True), outs) == plain
        assert outputs(mal.run_plan(ora, plan, env, fuse=True, hashed=True), outs) == plain


@pytest.mark.gpu
def test_hashed_plans_on_the_device(gdk, ora):
    """The rewritten plan on the product equals the plan as written on the
    product and on the oracle, output by output, and it is the hashed fused
    operator that ran it -- once per rewritten plan."""
    small = make_cols(5_003, 3, 8, 5)
    big = make_cols(70_001, 4, 24, 7)                         # 25 keys with the nil x 7 years
    cases = [(TWO_KEYS, TWO_OUTS, small, 5_003, 45), (ONE_KEY, ONE_OUTS, small, 5_003, 5),
             (TWO_KEYS, TWO_OUTS, big, 70_001, 175)]
    gdk.prof_enable(True)
    try:
        for plan, outs, (h, types), n, ng in cases:
            ge, oe = env_of(gdk, h, types, n), env_of(ora, h, types, n)
            want = outputs(mal.run_plan(ora, plan, oe, fuse=False), outs)
            assert len(want["n"]) == ng
            before = gdk.prof_get("select_groupsum_hash_fused")[1]
            narrow = gdk.prof_get("select_groupsum_fused")[1]
            plain = outputs(mal.run_plan(gdk, plan, ge, fuse=False), outs)
            assert gdk.prof_get("select_groupsum_hash_fused")[1] == before
            rewritten = mal.fuse_select_groupsum(plan)
            assert [fn for _, fn, _ in rewritten] == ["mgdk.select_groupsum"]
            fused = outputs(mal.run_plan(gdk, rewritten, ge, hashed=True), outs)
            assert gdk.prof_get("select_groupsum_hash_fused")[1] == before + 1
            assert gdk.prof_get("select_groupsum_fused")[1] == narrow      # wider keys go to the hashed entry at once
            for k in outs:
                assert fused[k] == plain[k] == want[k], k
    finally:
        gdk.prof_enable(False)


@pytest.mark.gpu
def test_q1_stays_with_the_narrow_entry(gdk, ora):
    import test_mal_fuse_group as narrow
    n = 100_003
    host = ora.tpch_lineitem(5, 0, n, 20_000)
    cols = gdk.tpch_lineitem(5, 0, n, 20_000)
    plan = narrow.q1_plan(ora.mkdate(1998, 9, 2))
    want = narrow.outputs(mal.run_plan(ora, plan, narrow.q1_env(ora, host), fuse=False), narrow.Q1_OUTS)
    gdk.prof_enable(True)
    try:
        a, b = gdk.prof_get("select_groupsum_fused")[1], gdk.prof_get("select_groupsum_hash_fused")[1]
        got = narrow.outputs(mal.run_plan(gdk, plan, narrow.q1_env(gdk, None, cols), hashed=True), narrow.Q1_OUTS)
        assert gdk.prof_get("select_groupsum_fused")[1] == a + 1
        assert gdk.prof_get("select_groupsum_hash_fused")[1] == b
    finally:
        gdk.prof_enable(False)
    assert got == want


@pytest.mark.gpu
def test_300_groups_run_the_kept_instructions(gdk, ora):
    n = 70_001
    h, types = make_cols(n, 6, 24, 12)
    ge, oe = env_of(gdk, h, types, n), env_of(ora, h, types, n)
    want = outputs(mal.run_plan(ora, TWO_KEYS, oe, fuse=False), TWO_OUTS)
    assert len(want["n"]) == 300
    assert outputs(mal.run_plan(gdk, TWO_KEYS, ge, hashed=True), TWO_OUTS) == want
