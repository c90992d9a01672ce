"""gdk.select_groupsum: the fused select cascade + GROUP BY sums against three
references that must agree bit for bit -- the same chain through the oracle's
operators, through the device operators (fused=False), and a model in plain
Python integers."""
import functools

import numpy as np
import pytest

HGE_NIL = -(1 << 127)
LNG_MAX = (1 << 63) - 1
NP = {"bte": np.int8, "sht": np.int16, "int": np.int32, "lng": np.int64, "date": np.int32}
SIZES = (1, 255, 256, 257, 511, 513, 2_049, 70_001)


def tnil(t):
    return int(np.iinfo(NP[t]).min)


# ---- the three references --------------------------------------------------------
# cols: {name: (type name, values)}; preds: (column, val, op) or (column, lo, hi, li, hi, anti);
# keys: column names; sums: tuples of factors, a factor a column name or (op, cst, column)

def pred_mask(cols, p):
    t, v = cols[p[0]]
    v = v.astype(object)
    ok = np.array([x != tnil(t) for x in v], bool)
    if len(p) == 3:
        f = {"<": lambda x: x < p[1], "<=": lambda x: x <= p[1], ">": lambda x: x > p[1], ">=": lambda x: x >= p[1],
             "==": lambda x: x == p[1], "!=": lambda x: x != p[1]}[p[2]]
        return ok & np.array([f(x) for x in v], bool)
    lo, hi, li, hi_inc, anti = p[1:6]
    assert not anti
    return ok & np.array([(x >= lo if li else x > lo) and (x <= hi if hi_inc else x < hi) for x in v], bool)


def factor_parts(f):
    return (None, 0, f) if isinstance(f, str) else f


def model(cols, preds, keys, sums, lo=0, hi=None, base=0):
    """Groups by first occurrence among the surviving rows of [lo, hi)."""
    n = len(next(iter(cols.values()))[1])
    hi = n if hi is None else hi
    live = np.zeros(n, bool)
    live[lo:hi] = True
    for p in preds:
        live &= pred_mask(cols, p)
    groups, order = {}, []
    for i in np.flatnonzero(live):
        k = tuple(int(cols[c][1][i]) & 0xff for c in keys)
        if k not in groups:
            groups[k] = dict(first=base + int(i), keys=k, count=0, sums=[0] * len(sums), nonnil=[0] * len(sums))
            order.append(k)
        g = groups[k]
        g["count"] += 1
        for j, fs in enumerate(sums):
            term = 1
            for f in fs:
                op, cst, c = factor_parts(f)
                x = int(cols[c][1][i])
                if x == tnil(cols[c][0]):
                    term = None
                    break
                term *= cst + x if op == "+" else cst - x if op == "-" else x
            if term is not None:
                g["sums"][j] += term
                g["nonnil"][j] += 1
    out = [groups[k] for k in order]
    for g in out:
        g["sums"] = [s if nn else None for s, nn in zip(g["sums"], g["nonnil"])]
    return out, live


def in_scope(cols, sums, live):
    """The bound of the overflow rule in plain integers: every cst +- col
    factor within +-(2^63 - 1) over the surviving non-nil rows, and survivors
    x the product of the factors' largest magnitudes below 2^127."""
    rows = int(live.sum())
    for fs in sums:
        b = rows
        for f in fs:
            op, cst, c = factor_parts(f)
            t, v = cols[c]
            vals = [int(x) for x in v[live] if int(x) != tnil(t)]
            if not vals:
                b = 0
                continue
            r = [cst + min(vals), cst + max(vals)] if op == "+" else [cst - max(vals), cst - min(vals)] if op == "-" \
                else [min(vals), max(vals)]
            if op and (r[0] < -LNG_MAX or r[1] > LNG_MAX):
                return False
            b *= max(abs(r[0]), abs(r[1]))
        if b >= 1 << 127:
            return False
    return True


def bind(mod, cols, hseqbase=0):
    mk = mod.BAT.from_numpy if hasattr(mod, "BAT") else mod.Bat.from_array
    return {k: mk(getattr(mod, "TYPE_" + t), v, hseqbase=hseqbase) for k, (t, v) in cols.items()}


def ora_chain(ora, env, preds, keys, sums, s=None):
    """The fragment through the oracle's operators, as the issue's chain."""
    c = s
    for p in preds:
        b = env[p[0]]
        c = ora.BATthetaselect(b, c, p[1], p[2]) if len(p) == 3 else ora.BATselect(b, c, *p[1:6])
    k = [ora.BATproject(c, env[x]) for x in keys]
    g, e, h = ora.BATgroup(k[0])
    if len(k) > 1:
        g, e, h = ora.BATgroup(k[1], None, g)
    svals, nvals = [], []
    for fs in sums:
        x = None
        for f in fs:
            op, cst, col = factor_parts(f)
            v = ora.BATproject(c, env[col])
            if op:
                v = ora.BATcalc(op, None, v, ora.TYPE_lng, c1=cst, t1=ora.TYPE_lng)
            x = v if x is None else ora.BATcalc("*", x, v, ora.TYPE_hge)
        svals.append(ora.BATgroupsum(x, g, e, ora.TYPE_hge, True).values())
        nvals.append(ora.BATgroupcount(x, g, e, True).values())
    cnt = ora.BATgroupcount(k[0], g, e, False).values()
    first = ora.BATproject(e, c).values()
    kv = [ora.BATproject(e, x).values() for x in k]
    out = []
    for i in range(e.count()):
        ss = [int(sv[i]) for sv in svals]
        out.append(dict(first=int(first[i]), keys=tuple(int(x[i]) & 0xff for x in kv), count=int(cnt[i]),
                        sums=[None if v == HGE_NIL else v for v in ss], nonnil=[int(nv[i]) for nv in nvals]))
    return out


def bound(env, preds, keys, sums):
    return ([(env[p[0]],) + tuple(p[1:]) for p in preds], [env[k] for k in keys],
            [tuple(env[f] if isinstance(f, str) else (f[0], f[1], env[f[2]]) for f in fs) for fs in sums])


def check_all(gdk, ora, cols, preds, keys, sums, s=None, want_fused=True):
    """Model == oracle chain == device operators == fused (which must have run)."""
    lo, hi = (0, None) if s is None else s
    want, live = model(cols, preds, keys, sums, lo, hi)
    assert in_scope(cols, sums, live) == want_fused
    oenv, genv = bind(ora, cols), bind(gdk, cols)
    os_ = gs = None
    if s is not None:
        os_, gs = ora.Bat.dense(lo, hi - lo), gdk.BAT.dense(lo, hi - lo)
    assert ora_chain(ora, oenv, preds, keys, sums, os_) == want
    gp, gk, gsum = bound(genv, preds, keys, sums)
    got, used = gdk.select_groupsum(gp, gk, gsum, gs, fused=False)
    assert not used and got == want
    got, used = gdk.select_groupsum(gp, gk, gsum, gs, fused=True)
    assert used == want_fused, "an in-scope request was declared not applicable" if want_fused else "fused"
    assert got == want
    return want


# ---- generated cases ---------------------------------------------------------------

PREDS = [("p0", 3, 17, True, False, False), ("p1", 5, "!=")]
SUMS = [("v1",), ("v2",), ("v4",), ("v8",), ("v8", ("-", 100, "v4")), (("+", 7, "v1"), "v2", "v8")]


@functools.lru_cache(maxsize=None)
def make_case(n, seed=0):
    r = np.random.default_rng(100 + n + seed)
    cols = {"p0": ("int", r.integers(0, 20, n).astype(np.int32)), "p1": ("sht", r.integers(0, 9, n).astype(np.int16)),
            "k0": ("bte", r.choice(np.array([1, 2, 3, -128], np.int8), n)),
            "k1": ("bte", r.integers(0, 2, n).astype(np.int8)),
            "v1": ("bte", r.integers(-100, 100, n).astype(np.int8)),
            "v2": ("sht", r.integers(-30000, 30000, n).astype(np.int16)),
            "v4": ("int", r.integers(-(1 << 30), 1 << 30, n).astype(np.int32)),
            "v8": ("lng", r.integers(-(1 << 40), 1 << 40, n).astype(np.int64))}
    for c in ("p0", "p1", "v1", "v2", "v4", "v8"):
        t, v = cols[c]
        v[r.random(n) < 0.03] = tnil(t)
    return cols


@pytest.mark.gpu
@pytest.mark.parametrize("nkeys", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_generated(gdk, ora, n, nkeys):
    """Every row count around the chunk and workgroup edges; one and two bte
    keys with nils; sums of every width, products of 2 and 3 factors mixing
    widths, both affine forms, nils in every factor."""
    cols = make_case(n)
    want = check_all(gdk, ora, cols, PREDS, ["k0", "k1"][:nkeys], SUMS)
    if n >= 2_049:
        assert len(want) == (4, 8)[nkeys - 1]        # the nil key is a key; exactly 8 groups fuse


def placed_case():
    n = 70_001
    cols = {k: (t, v.copy()) for k, (t, v) in make_case(n, 1).items()}
    p0, k0, v8 = cols["p0"][1], cols["k0"][1], cols["v8"][1]
    k0[:] = 1
    p0[:] = 10
    p0[::7] = 0                       # filtered
    k0[0:10] = 5; p0[0:10] = 0        # key 5: its earliest rows are filtered out ...
    k0[10] = 5; p0[10] = 10           # ... its first survivor is row 10
    k0[20_000:20_050] = 9; p0[20_000:20_050] = 0     # key 9 never survives
    k0[3_000] = 4; p0[3_000] = 10     # first rows in different workgroups, in this order
    k0[40_001] = 6; p0[40_001] = 10
    k0[n - 1] = 7; p0[n - 1] = 10     # only in the last, partial chunk
    k0[50_000:50_100] = 3             # a group whose every v8 is nil
    v8[k0 == 3] = tnil("lng")
    p0[50_003] = 10
    return cols


@pytest.mark.gpu
def test_group_placement(gdk, ora):
    cols = placed_case()
    n = 70_001
    want = check_all(gdk, ora, cols, [("p0", 3, 17, True, False, False)], ["k0"], SUMS)
    assert [g["keys"][0] for g in want] == [5, 1, 4, 6, 3, 7]          # first-occurrence order
    by = {g["keys"][0]: g for g in want}
    assert by[5]["first"] == 10 and by[4]["first"] == 3_000 and by[6]["first"] == 40_001 and by[7]["first"] == n - 1
    assert 9 not in by
    assert by[3]["sums"][3] is None and by[3]["nonnil"][3] == 0 and by[3]["count"] > 0
    assert by[3]["sums"][0] is not None


@pytest.mark.gpu
def test_group_limit(gdk, ora):
    """Exactly 8 groups are fused (test_generated); a ninth leaves the request to the operators."""
    n = 2_049
    cols = {k: (t, v.copy()) for k, (t, v) in make_case(n).items()}
    cols["k0"][1][n - 1] = 77
    cols["p0"][1][n - 1] = 10
    cols["p1"][1][n - 1] = 1
    want, live = model(cols, PREDS, ["k0", "k1"], SUMS)
    assert len(want) == 9 and in_scope(cols, SUMS, live)
    gp, gk, gs = bound(bind(gdk, cols), PREDS, ["k0", "k1"], SUMS)
    gdk.lib().mgdk_GDKclrerr()
    assert gdk.select_groupsum(gp, gk, gs, fallback=False) is None
    assert gdk.lib().mgdk_GDKerrbuf() == b""
    assert gdk.select_groupsum(gp, gk, gs) == (want, False)
    assert ora_chain(ora, bind(ora, cols), PREDS, ["k0", "k1"], SUMS) == want
    # no predicate at all: the groups of every row
    want, live = model(cols, [], ["k1"], SUMS[:2])
    assert gdk.select_groupsum([], [gk[1]], gs[:2]) == (want, True)


@pytest.mark.gpu
def test_str_keys_and_many_tracked_columns(gdk, ora):
    """str keys of one-byte offsets (the generated lineitem's flags), and 18
    lng columns in triple products: each keeps its minimum and maximum, which
    takes more LDS than the default limit."""
    n = 2_049
    dev = gdk.tpch_lineitem(3, 0, n, 20_000)
    host = ora.tpch_lineitem(3, 0, n, 20_000)
    r = np.random.default_rng(8)
    cols = {"shipdate": ("date", host["shipdate"]), "returnflag": ("bte", host["returnflag"].view(np.int8)),
            "linestatus": ("bte", host["linestatus"].view(np.int8))}
    for i in range(18):
        cols[f"x{i}"] = ("lng", r.integers(-1000, 1000, n).astype(np.int64))
    preds = [("shipdate", int(np.median(host["shipdate"])), "<=")]
    keys = ["returnflag", "linestatus"]
    sums = [tuple(f"x{3 * j + q}" for q in range(3)) for j in range(6)]
    want, live = model(cols, preds, keys, sums)
    assert in_scope(cols, sums, live) and 2 <= len(want) <= 8
    assert ora_chain(ora, bind(ora, cols), preds, keys, sums) == want
    genv = bind(gdk, {k: v for k, v in cols.items() if k not in keys})
    genv.update(returnflag=dev["returnflag"], linestatus=dev["linestatus"], shipdate=dev["shipdate"])
    assert genv["returnflag"].ttype == gdk.TYPE_str
    gp, gk, gs = bound(genv, preds, keys, sums)
    assert gdk.select_groupsum(gp, gk, gs, fused=False) == (want, False)
    assert gdk.select_groupsum(gp, gk, gs) == (want, True)


def lines_touched(mask, width):
    return len(np.unique(np.flatnonzero(mask) * width // 128))


@pytest.mark.gpu
def test_late_materialisation_is_real(gdk):
    """select_groupsum_last_lines counts, for every column after the first
    predicate's -- the keys included -- the 128-byte lines holding a row that
    passed everything before the column's first use."""
    n = 262_144
    r = np.random.default_rng(11)
    first = np.arange(n, dtype=np.int32)                       # sorted: one contiguous 10 % survives
    cols = {"first": ("int", first), "k": ("sht", r.integers(0, 10, n).astype(np.int16)),
            "g": ("bte", r.integers(0, 3, n).astype(np.int8)), "x": ("lng", r.integers(1, 1 << 30, n).astype(np.int64)),
            "y": ("int", r.integers(-100, 100, n).astype(np.int32))}
    lo, hi = n // 3, n // 3 + n // 10
    preds = [("first", lo, hi, True, False, False), ("k", 2, "<=")]
    sums = [("x", "k"), ("y",), ("x", ("-", 100, "y"))]
    want, live = model(cols, preds, ["g"], sums)
    m1 = (first >= lo) & (first < hi)
    assert (live == (m1 & (cols["k"][1] <= 2))).all()
    want_lines = lines_touched(m1, 2) + lines_touched(live, 1) + lines_touched(live, 8) + lines_touched(live, 4)
    gp, gk, gs = bound(bind(gdk, cols), preds, ["g"], sums)
    assert gdk.select_groupsum(gp, gk, gs) == (want, True)
    got = gdk.select_groupsum_last_lines()
    assert got == want_lines
    assert got < (2 + 1 + 8 + 4) * n // 128 // 5               # far below reading the columns whole


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["dense_cand", "slices", "aligned_slices"])
def test_candidates_and_views(gdk, ora, how):
    """A dense candidate list starting mid-column and BATslice views (heaps
    that are not 16-byte aligned) take the guarded loads; a slice starting
    16-byte aligned takes the buffer loads."""
    n = 70_001
    cols = make_case(n)
    keys = ["k0", "k1"]
    if how == "dense_cand":
        check_all(gdk, ora, cols, PREDS, keys, SUMS, s=(123, n - 77))
        return
    a, b = (3, n - 5) if how == "slices" else (16, n - 5)
    want, _ = model(cols, PREDS, keys, SUMS, a, b)
    genv = {k: gdk.BATslice(v, a, b) for k, v in bind(gdk, cols).items()}
    assert genv["v8"].hseqbase == a
    gp, gk, gs = bound(genv, PREDS, keys, SUMS)
    assert gdk.select_groupsum(gp, gk, gs) == (want, True)
    assert gdk.select_groupsum(gp, gk, gs, fused=False) == (want, False)
    oenv = bind(ora, {k: (t, v[a:b]) for k, (t, v) in cols.items()}, a)
    assert ora_chain(ora, oenv, PREDS, keys, SUMS) == want


@pytest.mark.gpu
def test_overflow_stays_with_the_operators(gdk, ora):
    big = 1 << 62

    def case(a, b, p, k):
        m = len(a)
        return {"p": ("int", np.array(p, np.int32)), "k": ("bte", np.array(k, np.int8)),
                "a": ("lng", np.array(a, np.int64)), "b": ("lng", np.array(b, np.int64))}

    preds, keys = [("p", 0, ">")], ["k"]
    # 100 - col with a surviving col = -(2^63 - 1) leaves lng: declined, and the operators raise
    sums = [(("-", 100, "a"),)]
    cols = case([5, -LNG_MAX, 7, 9], [1] * 4, [1, 1, 1, 1], [1, 2, 1, 2])
    _, live = model(cols, preds, keys, [])
    assert not in_scope(cols, sums, live)
    gp, gk, gs = bound(bind(gdk, cols), preds, keys, sums)
    assert gdk.select_groupsum(gp, gk, gs, fallback=False) is None
    with pytest.raises(ora.OracleError) as oe:
        ora_chain(ora, bind(ora, cols), preds, keys, sums)
    with pytest.raises(gdk.GDKError) as ge:
        gdk.select_groupsum(gp, gk, gs)
    assert str(ge.value) == str(oe.value)
    # the same value on a row the cascade removes decides nothing: fused
    cols = case([5, -LNG_MAX, 7, 9], [1] * 4, [1, 0, 1, 1], [1, 2, 1, 2])
    check_all(gdk, ora, cols, preds, keys, sums)
    # +-2^62 x 2^62 over 64 rows cancel to 0, but the sum of |term| is 2^130: declined
    sums = [("a", "b")]
    cols = case([big, -big] * 32, [big] * 64, [1] * 64, [1, 1, 2, 2] * 16)
    want = check_all(gdk, ora, cols, preds, keys, sums, want_fused=False)
    assert [g["sums"] for g in want] == [[0], [0]]
    # one such row per group: fused and exact
    cols = case([big, -big, big], [big] * 3, [1] * 3, [1, 2, 3])
    want = check_all(gdk, ora, cols, preds, keys, sums)
    assert [g["sums"][0] for g in want] == [1 << 124, -(1 << 124), 1 << 124]
    # sums beyond 2^64 in magnitude, of both signs: the carry into the high word
    m = 3_000
    cols = case([(1 << 40) + i for i in range(m)], [(-1) ** (i % 2) * ((1 << 30) + i) for i in range(m)],
                [1] * m, [i % 2 for i in range(m)])
    want = check_all(gdk, ora, cols, preds, keys, [("a", "b"), ("a",), ("b", "b", "a")])
    assert all(abs(g["sums"][0]) > 1 << 64 and abs(g["sums"][2]) > 1 << 64 for g in want)
    assert {g["sums"][0] < 0 for g in want} == {True, False}


@pytest.mark.gpu
def test_q1_is_an_instance(gdk, ora):
    n = 100_003
    cols = gdk.tpch_lineitem(7, 0, n, 20_000)
    host = ora.tpch_lineitem(7, 0, n, 20_000)
    dmax = ora.mkdate(1998, 9, 2)
    hc = {k: ("date" if k == "shipdate" else "lng", host[k]) for k in ("shipdate", "quantity", "extendedprice",
                                                                      "discount", "tax")}
    qty, price, disc, tax = (cols[k] for k in ("quantity", "extendedprice", "discount", "tax"))
    spec = [(qty,), (price,), (price, ("-", 100, disc)), (price, ("-", 100, disc), ("+", 100, tax)), (disc,)]
    names = [("quantity",), ("extendedprice",), ("extendedprice", ("-", 100, "discount")),
             ("extendedprice", ("-", 100, "discount"), ("+", 100, "tax")), ("discount",)]
    live = host["shipdate"] <= dmax
    assert in_scope(hc, names, live)
    got, used = gdk.select_groupsum([(cols["shipdate"], dmax, "<=")], [cols["returnflag"], cols["linestatus"]], spec)
    assert used
    ops, used = gdk.select_groupsum([(cols["shipdate"], dmax, "<=")], [cols["returnflag"], cols["linestatus"]], spec,
                                    fused=False)
    assert not used and ops == got
    q1 = sorted(gdk.q1_fused(cols, dmax), key=lambda r: (r["returnflag"], r["linestatus"]))
    oq1 = sorted(ora.q1(host, 1), key=lambda r: (r["returnflag"], r["linestatus"]))
    mine = sorted(got, key=lambda g: g["keys"])
    assert len(mine) == len(q1) == len(oq1) >= 3
    for g, r, o in zip(mine, q1, oq1):
        assert g["keys"] == (r["returnflag"], r["linestatus"]) == (o["returnflag"], o["linestatus"])
        assert g["sums"] == [r["sum_qty"], r["sum_base_price"], r["sum_disc_price"], r["sum_charge"], r["sum_disc"]]
        assert g["sums"][:4] == [o["sum_qty"], o["sum_base_price"], o["sum_disc_price"], o["sum_charge"]]
        assert g["count"] == r["count_order"] == o["count_order"] and g["first"] == r["first_row"]
        for j, k in ((0, "qty"), (1, "price"), (4, "disc")):
            assert gdk.avg3_of_sum(g["sums"][j], g["nonnil"][j]) == (r["avg_" + k], r["rem_" + k]) \
                == (o["avg_" + k], o["rem_" + k])
