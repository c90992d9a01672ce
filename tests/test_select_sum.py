"""gdk.select_sum: the fused select cascade + exact sums against the same
chain through the device operators and through the oracle, bit for bit."""
import functools

import numpy as np
import pytest

HGE_NIL = -(1 << 127)
TYPES = {"bte": np.int8, "sht": np.int16, "int": np.int32, "lng": np.int64, "date": np.int32}
SIZES = (0, 1, 255, 256, 257, 70_001)
NCASES = 42
THETA_OPS = ("eq", "ne", "==", "=", "!=", "<>", "<", "<=", ">", ">=")


def tnil(tname):
    return int(np.iinfo(TYPES[tname]).min)


def pred_kinds():
    """Every shape of predicate arguments the cases walk through: the 16
    li / hi / anti / nil_matches combinations of a plain range, the special
    bounds (each with two flag sets) and every thetaselect operator."""
    kinds = [("range", li, hi, anti, nm) for li in (0, 1) for hi in (0, 1) for anti in (0, 1) for nm in (0, 1)]
    for k in ("nil_low", "nil_high", "nil_both", "equal", "point", "point_nil", "type_min", "type_max",
              "type_both"):
        kinds += [(k, 1, 1, 0, 0), (k, 1, 0, 1, 1), (k, 0, 1, 1, 0), (k, 1, 1, 0, 1)]
    kinds += [("theta", op) for op in THETA_OPS] + [("theta_nil", "<"), ("theta_nil", "ne"), ("theta_nil", "eq")]
    return kinds


def pred_args(kind, tname):
    """The arguments after the column: (tl, th, li, hi, anti, nil_matches) or (val, op)."""
    nil, tmin, tmax = tnil(tname), tnil(tname) + 1, int(np.iinfo(TYPES[tname]).max)
    if kind[0] == "theta":
        return (7, kind[1])
    if kind[0] == "theta_nil":
        return (nil, kind[1])
    lo, hi = {"range": (3, 14), "nil_low": (nil, 12), "nil_high": (5, nil), "nil_both": (nil, nil),
              "equal": (7, 7), "point": (7, None), "point_nil": (nil, None), "type_min": (tmin, 12),
              "type_max": (5, tmax), "type_both": (tmin, tmax)}[kind[0]]
    return (lo, hi) + tuple(bool(f) for f in kind[1:])


@functools.lru_cache(maxsize=None)
def make_case(seed):
    """(columns {name: (type name, values)}, preds [(column, args...)], sums [(a, b | None)])"""
    r = np.random.default_rng(1000 + seed)
    n = SIZES[seed % len(SIZES)]
    kinds = pred_kinds()
    tnames = list(TYPES)
    cols, preds, sums = {}, [], []
    npreds = [1 + (s // len(SIZES)) % 4 for s in range(seed + 1)]
    npred, before = npreds[seed], sum(npreds[:seed])
    for i in range(npred):
        t = tnames[(seed + 2 * i) % len(tnames)]
        v = r.integers(0, 20, n).astype(TYPES[t])
        v[r.random(n) < 0.02] = tnil(t)
        cols[f"p{i}"] = (t, v)
        kind = kinds[(before + i) % len(kinds)]           # the cases walk through every shape in turn
        preds.append((f"p{i}",) + pred_args(kind, t))
    for j in range(4):
        t = tnames[(seed + j) % 4]
        v = r.integers(-50, 50, n).astype(TYPES[t])
        v[r.random(n) < 0.02] = tnil(t)
        cols[f"v{j}"] = (t, v)
    names = list(cols)
    for j in range(seed % 5):
        a = names[int(r.integers(len(names)))]
        b = names[int(r.integers(len(names)))] if r.random() < 0.6 else None
        sums.append((a, b))
    return cols, preds, sums


def bind(mod, cols, hseqbase=0):
    if hasattr(mod, "BAT"):
        return {k: mod.BAT.from_numpy(getattr(mod, "TYPE_" + t), v, hseqbase=hseqbase) for k, (t, v) in cols.items()}
    return {k: mod.Bat.from_array(getattr(mod, "TYPE_" + t), v, hseqbase=hseqbase) for k, (t, v) in cols.items()}


def bound(env, preds, sums):
    return ([(env[p[0]],) + tuple(p[1:]) for p in preds],
            [(env[a], env[b] if b is not None else None) for a, b in sums])


def ora_chain(ora, preds, sums, s=None):
    """The fragment through the oracle's operators: (sums, count)."""
    c = s
    for p in preds:
        c = ora.BATthetaselect(p[0], c, p[1], p[2]) if len(p) == 3 else ora.BATselect(p[0], c, *p[1:])
    out = []
    for a, b in sums:
        v = ora.BATproject(c, a)
        if b is not None:
            v = ora.BATcalc("*", v, ora.BATproject(c, b), ora.TYPE_hge)
        x = ora.BATsum(ora.TYPE_hge, v)
        out.append(None if x == HGE_NIL else x)
    return out, int(c.count())


@functools.lru_cache(maxsize=None)
def case_reference(seed):
    from oracle import pyoracle as ora
    cols, preds, sums = make_case(seed)
    p, s = bound(bind(ora, cols), preds, sums)
    return ora_chain(ora, p, s)


def test_generated_cases_are_in_scope(ora):
    """No generated case overflows in the oracle (so the fused path may take
    every one), every predicate shape is used, and survivors are common."""
    used, kept = set(), 0
    for seed in range(NCASES):
        cols, preds, sums = make_case(seed)
        sums_, cnt = case_reference(seed)          # raises on an overflow
        assert len(sums_) == len(sums) <= 4 and 1 <= len(preds) <= 4
        kept += cnt > 0
        used |= {tuple(p[1:]) if len(p) == 3 else tuple(p[3:]) + (p[1] == p[2], p[2] is None) for p in preds}
    assert kept >= NCASES // 3
    assert {(7, op) for op in THETA_OPS} <= used
    assert {(li, hi, anti, nm, False, False) for li in (False, True) for hi in (False, True)
            for anti in (False, True) for nm in (False, True)} <= used


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(NCASES))
def test_random_plans(gdk, ora, seed):
    cols, preds, sums = make_case(seed)
    p, s = bound(bind(gdk, cols), preds, sums)
    want = case_reference(seed)
    vals, cnt, used = gdk.select_sum(p, s, fused=True)
    assert used, "an in-scope request was declared not applicable"
    assert (vals, cnt) == want
    vals, cnt, used = gdk.select_sum(p, s, fused=False)
    assert not used and (vals, cnt) == want


@pytest.mark.gpu
def test_every_predicate_shape(gdk, ora):
    """Each shape of predicate arguments on each column type, as the second
    predicate of a cascade over 1 000 rows (the random cases meet some shapes
    only on their tiny sizes)."""
    n = 1_000
    r = np.random.default_rng(21)
    cols = {"first": ("int", r.integers(0, 20, n).astype(np.int32)), "v": ("lng", r.integers(-50, 50, n))}
    for t in TYPES:
        v = r.integers(0, 20, n).astype(TYPES[t])
        v[r.random(n) < 0.03] = tnil(t)
        cols[t] = (t, v)
    genv, oenv = bind(gdk, cols), bind(ora, cols)
    tnames = list(TYPES)
    for q, kind in enumerate(pred_kinds()):
        for t in (tnames[q % 5], tnames[(q + 2) % 5]):
            preds = [("first", 2, ">="), (t,) + pred_args(kind, t)]
            sums = [("v", t), ("v", None)]
            gp, gs = bound(genv, preds, sums)
            op, os_ = bound(oenv, preds, sums)
            assert gdk.select_sum(gp, gs) == ora_chain(ora, op, os_) + (True,), (kind, t)


def q6_preds(env, d0, d1):
    return [(env["shipdate"], d0, d1, True, False, False), (env["discount"], 5, 7, True, True, False),
            (env["quantity"], 2400, "<")]


@pytest.mark.gpu
@pytest.mark.parametrize("prices", ["generated", "near_2_60"])
def test_q6_is_an_instance(gdk, ora, prices):
    n = 1_000_003
    cols = gdk.tpch_lineitem(9, 0, n, 20_000)
    host = ora.tpch_lineitem(9, 0, n, 20_000)
    if prices == "near_2_60":                     # products beyond 64 bits
        host["extendedprice"][::61] = (1 << 60) + 7
        host["extendedprice"][1::67] = -(1 << 60) - 3
        cols["extendedprice"] = gdk.BAT.from_numpy(gdk.TYPE_lng, host["extendedprice"])
    d0, d1 = ora.mkdate(1994, 1, 1), ora.mkdate(1995, 1, 1)
    vals, cnt, used = gdk.select_sum(q6_preds(cols, d0, d1), [(cols["extendedprice"], cols["discount"])])
    assert used
    assert vals[0] == ora.q6(host, 4)
    assert vals[0] == gdk.q6_fused(cols["shipdate"], cols["discount"], cols["quantity"], cols["extendedprice"],
                                   d0, d1, 5, 7, 2400)
    sd, di, q = host["shipdate"], host["discount"], host["quantity"]
    assert cnt == int(((sd >= d0) & (sd < d1) & (di >= 5) & (di <= 7) & (q < 2400)).sum())


def view_case(n):
    r = np.random.default_rng(77)
    cols = {"d": ("date", r.integers(0, 30, n).astype(np.int32)), "k": ("sht", r.integers(0, 9, n).astype(np.int16)),
            "x": ("lng", r.integers(-(1 << 50), 1 << 50, n)), "y": ("bte", r.integers(-100, 100, n).astype(np.int8))}
    for t, v in cols.values():
        v[r.random(n) < 0.02] = tnil(t)
    preds = [("d", 4, 22, True, False, False, False), ("k", 3, "!="), ("y", tnil("bte"), 50, False, True, True, False)]
    sums = [("x", "y"), ("k", None), ("x", "d"), ("y", "y")]
    return cols, preds, sums


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["dense_cand", "slices", "hseqbase", "hseqbase_cand"])
def test_candidates_views_hseqbase(gdk, ora, how):
    n = 70_001
    cols, preds, sums = view_case(n)
    base = 1000 if how.startswith("hseqbase") else 0
    genv, oenv = bind(gdk, cols, base), bind(ora, cols, base)
    gs = os_ = None
    if how == "dense_cand":
        gs, os_ = gdk.BAT.dense(123, n - 200), ora.Bat.dense(123, n - 200)
    elif how == "hseqbase_cand":
        gs, os_ = gdk.BAT.dense(990, 5000), ora.Bat.dense(990, 5000)    # starts before the columns
    elif how == "slices":                          # views: heaps that are not 16-byte aligned
        genv = {k: gdk.BATslice(b, 3, n - 5) for k, b in genv.items()}
        oenv = bind(ora, {k: (t, v[3:n - 5]) for k, (t, v) in cols.items()}, 3)
        assert genv["x"].hseqbase == 3
    gp, gsum = bound(genv, preds, sums)
    op, osum = bound(oenv, preds, sums)
    want = ora_chain(ora, op, osum, os_)
    assert want[1] > 0
    vals, cnt, used = gdk.select_sum(gp, gsum, gs, fused=True)
    assert used and (vals, cnt) == want
    vals, cnt, used = gdk.select_sum(gp, gsum, gs, fused=False)
    assert not used and (vals, cnt) == want


@pytest.mark.gpu
def test_overflow_stays_with_the_operators(gdk, ora):
    big = 1 << 62

    def run(vals_a):
        m = len(vals_a)
        cols = {"p": ("int", np.ones(m, np.int32)), "a": ("lng", np.array(vals_a, np.int64)),
                "b": ("lng", np.full(m, big, np.int64))}
        preds, sums = [("p", 0, ">")], [("a", "b")]
        return bound(bind(gdk, cols), preds, sums), bound(bind(ora, cols), preds, sums)

    # A: 16 x 2^124 overflows the running sum: the operators' error, not a wrapped value
    (gp, gs), (op, os_) = run([big] * 16)
    assert gdk.select_sum(gp, gs, fallback=False) is None
    with pytest.raises(ora.OracleError) as oe:
        ora_chain(ora, op, os_)
    with pytest.raises(gdk.GDKError) as ge:
        gdk.select_sum(gp, gs)
    assert str(ge.value) == str(oe.value)
    # B: alternating signs over 64 rows: the true sum is 0 and no prefix overflows, but the
    # sum of |term| is 2^130 >= 2^127, so the fused path declines
    (gp, gs), (op, os_) = run([big, -big] * 32)
    assert ora_chain(ora, op, os_) == ([0], 64)
    assert gdk.select_sum(gp, gs) == ([0], 64, False)
    # C: the same over 4 rows, the sum of |term| = 2^126: fused and exact
    (gp, gs), (op, os_) = run([big, -big] * 2)
    assert gdk.select_sum(gp, gs) == ([0], 4, True) and ora_chain(ora, op, os_) == ([0], 4)
    (gp, gs), (op, os_) = run([big] * 4)
    assert gdk.select_sum(gp, gs) == ([1 << 126], 4, True) and ora_chain(ora, op, os_) == ([1 << 126], 4)


@pytest.mark.gpu
@pytest.mark.parametrize("why", ["dbl_predicate", "hge_operand", "materialised_cand", "different_counts",
                                 "five_predicates"])
def test_not_applicable_quietly(gdk, ora, why):
    n = 3_001
    r = np.random.default_rng(5)
    cols = {"p": ("int", r.integers(0, 20, n).astype(np.int32)), "v": ("lng", r.integers(-99, 99, n))}
    genv, oenv = bind(gdk, cols), bind(ora, cols)
    preds, sums = [("p", 3, 14, True, True, False, False)], [("v", "p"), ("v", None)]
    gs = os_ = None
    if why == "dbl_predicate":
        f = r.integers(0, 20, n).astype(np.float64)
        genv["f"], oenv["f"] = gdk.BAT.from_numpy(gdk.TYPE_dbl, f), ora.Bat.from_array(ora.TYPE_dbl, f)
        preds = preds + [("f", 2.0, 11.0, True, False, False, False)]
    elif why == "hge_operand":
        h = np.zeros((n, 2), np.uint64)
        h[:, 0] = r.integers(0, 1 << 40, n)
        genv["h"], oenv["h"] = gdk.BAT.from_numpy(gdk.TYPE_hge, h), ora.Bat.from_array(ora.TYPE_hge, h)
        sums = sums + [("h", None)]
    elif why == "materialised_cand":
        oids = np.flatnonzero(r.random(n) < 0.5).astype(np.uint64)
        gs = gdk.BAT.from_numpy(gdk.TYPE_oid, oids, sorted_=True, key=True)
        os_ = ora.Bat.from_array(ora.TYPE_oid, oids, sorted_=True, key=True, nonil=True)
    elif why == "different_counts":
        w = r.integers(-99, 99, n + 10)
        genv["v"], oenv["v"] = gdk.BAT.from_numpy(gdk.TYPE_lng, w), ora.Bat.from_array(ora.TYPE_lng, w)
    elif why == "five_predicates":
        preds = preds + [("p", k, ">") for k in (3, 4, 5, 6)]
    gp, gsum = bound(genv, preds, sums)
    op, osum = bound(oenv, preds, sums)
    gdk.lib().mgdk_GDKclrerr()
    assert gdk.select_sum(gp, gsum, gs, fallback=False) is None
    assert gdk.lib().mgdk_GDKerrbuf() == b""
    want = ora_chain(ora, op, osum, os_)
    assert want[1] > 0
    assert gdk.select_sum(gp, gsum, gs) == want + (False,)


def lines_touched(mask, width):
    return len(np.unique(np.flatnonzero(mask) * width // 128))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [262_144, 70_001])
def test_late_materialisation_is_real(gdk, n):
    """select_sum_last_lines counts, for every column after the first
    predicate's, the 128-byte lines holding a row that passed everything
    before the column's first use -- so only those lines were fetched."""
    r = np.random.default_rng(11)
    first = np.arange(n, dtype=np.int32)                       # sorted: one contiguous 10 % survives
    k = r.integers(0, 10, n).astype(np.int16)
    q = r.integers(0, 5000, n).astype(np.int64)
    x = r.integers(1, 1 << 30, n).astype(np.int64)
    y = r.integers(-100, 100, n).astype(np.int8)
    lo, hi = n // 3, n // 3 + n // 10
    B = {nm: gdk.BAT.from_numpy(getattr(gdk, "TYPE_" + t), v)
         for nm, (t, v) in dict(first=("int", first), k=("sht", k), q=("lng", q), x=("lng", x), y=("bte", y)).items()}
    preds = [(B["first"], lo, hi, True, False, False), (B["k"], 2, "<="), (B["q"], 2400, "<")]
    sums = [(B["x"], B["k"]), (B["y"], None), (B["x"], B["q"])]
    m1 = (first >= lo) & (first < hi)
    m2 = m1 & (k <= 2)
    m3 = m2 & (q < 2400)
    want_lines = lines_touched(m1, 2) + lines_touched(m2, 8) + lines_touched(m3, 8) + lines_touched(m3, 1)
    vals, cnt, used = gdk.select_sum(preds, sums)
    assert used and cnt == int(m3.sum())
    assert vals == [int((x[m3] * k[m3]).sum()), int(y[m3].astype(np.int64).sum()),
                    sum(int(a) * int(b) for a, b in zip(x[m3], q[m3]))]
    got = gdk.select_sum_last_lines()
    if n % 256 == 0:
        assert got == want_lines
    else:
        assert want_lines <= got <= want_lines + 4             # one line per later column for the tail
    assert got < (2 + 8 + 8 + 1) * n // 128 // 5               # far below reading the columns whole
