"""gdk.select_groupsum_hash: the fused select cascade + GROUP BY sums for keys
of up to 8 bytes together and up to 256 groups, against three references that
must agree bit for bit -- the same chain through the oracle's operators,
through the device operators (fused=False), and a model in plain Python
integers.  Keys are compared at their full width."""
import functools

import numpy as np
import pytest

HGE_NIL = -(1 << 127)
LNG_MAX = (1 << 63) - 1
I32_MAX, I64_MAX = (1 << 31) - 1, (1 << 63) - 1
NP = {"bte": np.int8, "sht": np.int16, "int": np.int32, "lng": np.int64, "date": np.int32}
SIZES = (1, 255, 256, 257, 511, 513, 2_049, 70_001)


def tnil(t):
    return int(np.iinfo(NP[t]).min)


# ---- the references ------------------------------------------------------------------
# cols: {name: (type name, values)}; preds: (column, val, op) or (column, lo, hi, li, hi, anti);
# keys: column names; sums: tuples of factors, a factor a column name or (op, cst, column)

def pred_mask(cols, p):
    t, v = cols[p[0]]
    v = v.astype(np.int64)
    ok = v != tnil(t)
    if len(p) == 3:
        f = {"<": v < p[1], "<=": v <= p[1], ">": v > p[1], ">=": v >= p[1], "==": v == p[1], "!=": v != p[1]}[p[2]]
        return ok & f
    lo, hi, li, hi_inc, anti = p[1:6]
    assert not anti
    return ok & (v >= lo if li else v > lo) & (v <= hi if hi_inc else v < hi)


def factor_parts(f):
    return (None, 0, f) if isinstance(f, str) else f


def model(cols, preds, keys, sums, lo=0, hi=None, base=0):
    """Groups by first occurrence among the surviving rows of [lo, hi); keys at full width."""
    n = len(next(iter(cols.values()))[1])
    hi = n if hi is None else hi
    live = np.zeros(n, bool)
    live[lo:hi] = True
    for p in preds:
        live &= pred_mask(cols, p)
    idx = np.flatnonzero(live)
    kv = [cols[c][1][idx].tolist() for c in keys]
    terms = []
    for fs in sums:
        t = [1] * len(idx)
        for f in fs:
            op, cst, c = factor_parts(f)
            nil = tnil(cols[c][0])
            xs = cols[c][1][idx].tolist()
            t = [None if (a is None or x == nil) else a * (cst + x if op == "+" else cst - x if op == "-" else x)
                 for a, x in zip(t, xs)]
        terms.append(t)
    groups, order = {}, []
    for pos, k in enumerate(zip(*kv)):
        g = groups.get(k)
        if g is None:
            g = groups[k] = dict(first=base + int(idx[pos]), keys=k, count=0, sums=[0] * len(sums),
                                 nonnil=[0] * len(sums))
            order.append(k)
        g["count"] += 1
        for j, t in enumerate(terms):
            if t[pos] is not None:
                g["sums"][j] += t[pos]
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
            vals = v[live]
            vals = vals[vals != tnil(t)]
            if not len(vals):
                b = 0
                continue
            mn, mx = int(vals.min()), int(vals.max())
            r = [cst + mn, cst + mx] if op == "+" else [cst - mx, cst - mn] if op == "-" else [mn, mx]
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
        out.append(dict(first=int(first[i]), keys=tuple(int(x[i]) for x in kv), count=int(cnt[i]),
                        sums=[None if v == HGE_NIL else v for v in ss], nonnil=[int(nv[i]) for nv in nvals]))
    return out


def bound(env, preds, keys, sums):
    return ([(env[p[0]],) + tuple(p[1:]) for p in preds], [env[k] for k in keys],
            [tuple(env[f] if isinstance(f, str) else (f[0], f[1], env[f[2]]) for f in fs) for fs in sums])


def errbuf_clean_none(gdk, *args, **kw):
    """fallback=False answers None and leaves no error text."""
    gdk.lib().mgdk_GDKclrerr()
    assert gdk.select_groupsum_hash(*args, fallback=False, **kw) is None
    assert gdk.lib().mgdk_GDKerrbuf() == b""


def check_all(gdk, ora, cols, preds, keys, sums, s=None, want_fused=True, genv=None, want=None):
    """Model == oracle chain == device operators == fused (which must have run)."""
    lo, hi = (0, None) if s is None else s
    if want is None:
        want = model(cols, preds, keys, sums, lo, hi)
    want, live = want
    assert in_scope(cols, sums, live) == want_fused
    oenv = bind(ora, cols)
    genv = bind(gdk, cols) if genv is None else genv
    os_ = gs = None
    if s is not None:
        os_, gs = ora.Bat.dense(lo, hi - lo), gdk.BAT.dense(lo, hi - lo)
    assert ora_chain(ora, oenv, preds, keys, sums, os_) == want
    gp, gk, gsum = bound(genv, preds, keys, sums)
    got, used = gdk.select_groupsum_hash(gp, gk, gsum, gs, fused=False)
    assert not used and got == want
    got, used = gdk.select_groupsum_hash(gp, gk, gsum, gs, fused=True)
    assert used == want_fused, "an in-scope request was declared not applicable" if want_fused else "fused"
    assert got == want
    return want


# ---- generated cases -------------------------------------------------------------------

PREDS = [("p0", 3, 17, True, False, False), ("p1", 5, "!=")]
SUMS = [("v1",), ("v2",), ("v4",), ("v8",), ("v8", ("-", 100, "v4")), (("+", 7, "v1"), "v2", "v8")]
KEY_FORMS = {"sht": ("ksht",), "int": ("kint",), "lng": ("klng",), "date": ("kdate",), "bte_int": ("kb", "kint"),
             "int_int": ("kint", "kint2"), "sht_bte": ("ksht", "kb"), "bte_bte": ("kb", "kb3")}


@functools.lru_cache(maxsize=None)
def make_case(n, seed=0):
    r = np.random.default_rng(4100 + n + seed)
    cols = {"p0": ("int", r.integers(0, 20, n).astype(np.int32)), "p1": ("sht", r.integers(0, 9, n).astype(np.int16)),
            "ksht": ("sht", r.choice(np.array([-5, 300, -32768, 7, 32767], np.int16), n)),
            "kint": ("int", r.choice(np.array([1995, -(1 << 31), I32_MAX, -1, 0, 70_000], np.int32), n)),
            "kint2": ("int", r.choice(np.array([0, -(1 << 31), 12], np.int32), n)),
            "klng": ("lng", r.choice(np.array([1 << 40, -(1 << 63), -1, 3, I64_MAX], np.int64), n)),
            "kdate": ("date", r.choice(np.array([727_000, 727_001, -(1 << 31), 730_000], np.int32), n)),
            "kb": ("bte", r.choice(np.array([1, 2, 3, -128], np.int8), n)),
            "kb3": ("bte", r.integers(0, 3, n).astype(np.int8)),
            "v1": ("bte", r.integers(-100, 100, n).astype(np.int8)),
            "v2": ("sht", r.integers(-30000, 30000, n).astype(np.int16)),
            "v4": ("int", r.integers(-(1 << 30), 1 << 30, n).astype(np.int32)),
            "v8": ("lng", r.integers(-(1 << 40), 1 << 40, n).astype(np.int64))}
    for c in ("p0", "p1", "v1", "v2", "v4", "v8"):
        t, v = cols[c]
        v[r.random(n) < 0.03] = tnil(t)
    return cols


@functools.lru_cache(maxsize=None)
def case_model(n, form):
    return model(make_case(n), PREDS, KEY_FORMS[form], SUMS)


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(KEY_FORMS))
@pytest.mark.parametrize("n", SIZES)
def test_generated(gdk, ora, n, form):
    """Every row count around the chunk and workgroup edges; keys of every
    width alone and in pairs, nil keys among them; sums of every width,
    products of 2 and 3 factors mixing widths, both affine forms, nils in
    every predicate and factor column."""
    want = check_all(gdk, ora, make_case(n), PREDS, KEY_FORMS[form], SUMS, want=case_model(n, form))
    if n >= 2_049:
        assert len(want) == {"sht": 5, "int": 6, "lng": 5, "date": 4, "bte_int": 24, "int_int": 18, "sht_bte": 20,
                             "bte_bte": 12}[form]


@pytest.mark.gpu
def test_the_narrow_limit_is_what_moved(gdk):
    """The data of test_select_groupsum.py::test_group_limit: nine groups on
    byte keys are beyond the narrow entry and within this one."""
    import test_select_groupsum as narrow
    n = 2_049
    cols = {k: (t, v.copy()) for k, (t, v) in narrow.make_case(n).items()}
    cols["k0"][1][n - 1] = 77
    cols["p0"][1][n - 1] = 10
    cols["p1"][1][n - 1] = 1
    want, live = model(cols, narrow.PREDS, ["k0", "k1"], narrow.SUMS)
    assert len(want) == 9 and in_scope(cols, narrow.SUMS, live)
    gp, gk, gs = bound(bind(gdk, cols), narrow.PREDS, ["k0", "k1"], narrow.SUMS)
    assert gdk.select_groupsum(gp, gk, gs, fallback=False) is None
    assert gdk.select_groupsum_hash(gp, gk, gs) == (want, True)
    assert gdk.select_groupsum_hash(gp, gk, gs, fallback=False) == (want, True)


def filtered_p0(n):
    p0 = np.full(n, 10, np.int32)
    p0[::7] = 0
    return p0


P0 = [("p0", 3, 17, True, False, False)]


@pytest.mark.gpu
def test_256_and_257_groups(gdk, ora):
    n = 2_049
    base = make_case(n)
    cols = {c: base[c] for c in ("v1", "v2", "v4", "v8")}
    cols["p0"] = ("int", filtered_p0(n))
    cols["k"] = ("int", ((np.arange(n) % 256) * 1_000_003 - 5).astype(np.int32))
    want = check_all(gdk, ora, cols, P0, ["k"], SUMS)
    assert len(want) == 256
    gp, gk, gs = bound(bind(gdk, cols), P0, ["k"], SUMS)
    # room for fewer groups than there are: not applicable, and the operators say so
    errbuf_clean_none(gdk, gp, gk, gs, maxgroups=255)
    with pytest.raises(gdk.GDKError):
        gdk.select_groupsum_hash(gp, gk, gs, maxgroups=255)
    # a 257th key on a surviving row
    cols["k"] = ("int", cols["k"][1].copy())
    cols["k"][1][n - 1] = 999
    assert cols["p0"][1][n - 1] == 10
    want, live = model(cols, P0, ["k"], SUMS)
    assert len(want) == 257 and in_scope(cols, SUMS, live)
    gp, gk, gs = bound(bind(gdk, cols), P0, ["k"], SUMS)
    errbuf_clean_none(gdk, gp, gk, gs, maxgroups=300)
    errbuf_clean_none(gdk, gp, gk, gs)
    assert gdk.select_groupsum_hash(gp, gk, gs, maxgroups=300) == (want, False)
    assert ora_chain(ora, bind(ora, cols), P0, ["k"], SUMS) == want


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["lng", "int_int"])
def test_every_marker_candidate_is_a_key(gdk, ora, form):
    """0, -1, nil, nil + 1, the maximum and 1 as keys; for two int keys every
    combination of 0, -1, nil and the maximum (code all ones and code 0
    among them).  Whatever value marks an empty entry is one of these."""
    n = 2_049
    base = make_case(n)
    cols = {c: base[c] for c in ("v1", "v2", "v4", "v8")}
    cols["p0"] = ("int", filtered_p0(n))
    i = np.arange(n)
    if form == "lng":
        vals = np.array([0, -1, -(1 << 63), -(1 << 63) + 1, I64_MAX, 1], np.int64)
        cols["k"] = ("lng", vals[i % 6])
        keys, ng = ["k"], 6
    else:
        half = np.array([0, -1, -(1 << 31), I32_MAX], np.int32)
        cols["k"] = ("int", half[i % 4])
        cols["j"] = ("int", half[(i // 4) % 4])
        keys, ng = ["k", "j"], 16
    want = check_all(gdk, ora, cols, P0, keys, SUMS)
    assert len(want) == ng and all(g["count"] > 20 for g in want)
    if form == "int_int":
        assert {(-1, -1), (0, 0)} <= {g["keys"] for g in want}


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["lng", "int_int"])
def test_marker_candidates_in_a_crowded_table(gdk, ora, form):
    """One chunk, one wave: the marker candidates sit on the rows a lane
    resolves first (4l), 192 other random keys on the rows it resolves after
    them.  If the code that marks an empty entry went through the probed
    table, its entry would still read as empty and a later key could claim
    it; over 10 draws of the other keys one of them does."""
    n = 256
    base = make_case(n)
    i = np.arange(n)
    for seed in range(10):
        r = np.random.default_rng(700 + seed)
        cols = {c: base[c] for c in ("v1", "v2", "v4", "v8")}
        cols["p0"] = ("int", np.where(i % 64 == 63, 0, 10).astype(np.int32))      # a few filtered rows
        if form == "lng":
            vals = np.array([0, -1, -(1 << 63), -(1 << 63) + 1, I64_MAX, 1], np.int64)
            k = r.integers(-(1 << 62), 1 << 62, n).astype(np.int64)
            k[::4] = vals[(i[::4] // 4) % 6]
            cols["k"] = ("lng", k)
            keys = ["k"]
        else:
            half = np.array([0, -1, -(1 << 31), I32_MAX], np.int32)
            k = r.integers(2, 1 << 30, n).astype(np.int32)
            j = r.integers(2, 1 << 30, n).astype(np.int32)
            k[::4] = half[(i[::4] // 4) % 4]
            j[::4] = half[(i[::4] // 16) % 4]
            cols["k"], cols["j"] = ("int", k), ("int", j)
            keys = ["k", "j"]
        want = check_all(gdk, ora, cols, P0, keys, SUMS[:4])
        assert 190 < len(want) <= 256


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["shift20", "shift32", "consecutive"])
def test_probing_under_clustering(gdk, ora, how):
    """256 groups whose codes differ in few bits: i << 20 (a hash of the low
    bits alone would put them all on one entry), i << 32 (two int keys, the
    low one constant) and consecutive integers."""
    n = 70_001
    base = make_case(n)
    cols = {c: base[c] for c in ("p0", "p1", "v1", "v2", "v4", "v8")}
    ids = np.random.default_rng(5).permutation(256)[np.random.default_rng(6).integers(0, 256, n)]
    if how == "shift20":
        cols["k"] = ("int", (ids << 20).astype(np.int32))
        keys = ["k"]
    elif how == "shift32":
        cols["c"] = ("int", np.full(n, 5, np.int32))
        cols["k"] = ("int", ids.astype(np.int32))
        keys = ["c", "k"]
    else:
        cols["k"] = ("int", (ids + 1000).astype(np.int32))
        keys = ["k"]
    want = check_all(gdk, ora, cols, PREDS, keys, SUMS[:3])
    assert len(want) == 256


def placed_case():
    n = 70_001
    base = make_case(n, 1)
    cols = {c: (t, v.copy()) for c, (t, v) in base.items() if c in ("v1", "v2", "v4", "v8")}
    keyvals = (np.random.default_rng(9).permutation(197) * 37 - 3000).astype(np.int32)
    k = keyvals[np.arange(n) % 197]
    p0 = filtered_p0(n)
    v8 = cols["v8"][1]
    A, B, C, D = 100_001, 100_002, 100_003, 100_004
    k[0:11] = A; p0[0:10] = 0; p0[10] = 10           # A: its earliest rows are filtered, first survivor row 10
    k[20_000:20_050] = B; p0[20_000:20_050] = 0      # B never survives
    k[n - 1] = C; p0[n - 1] = 10                     # C: only in the last, partial chunk
    k[50_000:50_100] = D; p0[50_003] = 10            # D: every v8 is nil
    v8[k == D] = tnil("lng")
    cols["k"] = ("int", k)
    cols["p0"] = ("int", p0)
    return cols, (A, B, C, D)


@pytest.mark.gpu
def test_group_placement(gdk, ora):
    cols, (A, B, C, D) = placed_case()
    n = 70_001
    want = check_all(gdk, ora, cols, P0, ["k"], SUMS)
    order = [g["keys"][0] for g in want]
    assert len(want) == 200 and order != sorted(order) and order[0] == A       # first-occurrence order, not key order
    assert [g["first"] for g in want] == sorted(g["first"] for g in want)
    by = {g["keys"][0]: g for g in want}
    assert by[A]["first"] == 10 and by[C]["first"] == n - 1 and order[-1] == C
    assert B not in by
    assert by[D]["sums"][3] is None and by[D]["nonnil"][3] == 0 and by[D]["count"] > 0
    assert by[D]["sums"][0] is not None


@pytest.mark.gpu
def test_merge_across_workgroups(gdk):
    """Every 8 192-row stretch holds all 256 groups, so every workgroup meets
    all of them and the merge adds 256 entries per workgroup.  Values small
    enough that an int64 model is exact."""
    n = 262_144
    r = np.random.default_rng(21)
    perm = r.permutation(256).astype(np.int64) * ((1 << 55) + 12_345) - (1 << 62)
    k = perm[np.arange(n) % 256]
    p0 = (np.arange(n) % 7).astype(np.int32)
    a = r.integers(-1000, 1000, n).astype(np.int32)
    b = r.integers(-1000, 1000, n).astype(np.int16)
    a[r.random(n) < 0.03] = tnil("int")
    cols = {"p0": ("int", p0), "k": ("lng", k), "a": ("int", a), "b": ("sht", b)}
    live = p0 != 0
    idx = np.flatnonzero(live)
    uk, first, inv = np.unique(k[idx], return_index=True, return_inverse=True)
    nn = a[idx] != tnil("int")
    cnt = np.bincount(inv, minlength=256)
    s = np.zeros((3, 256), np.int64)
    np.add.at(s[0], inv[nn], a[idx][nn].astype(np.int64))
    np.add.at(s[1], inv, b[idx].astype(np.int64))
    np.add.at(s[2], inv[nn], a[idx][nn].astype(np.int64) * b[idx][nn])
    nnc = np.bincount(inv[nn], minlength=256)
    want = [dict(first=int(idx[first[g]]), keys=(int(uk[g]),), count=int(cnt[g]),
                 sums=[int(s[0][g]), int(s[1][g]), int(s[2][g])], nonnil=[int(nnc[g]), int(cnt[g]), int(nnc[g])])
            for g in np.argsort(first)]
    assert len(want) == 256 and want[0]["first"] == 1
    gp, gk, gs = bound(bind(gdk, cols), [("p0", 0, "!=")], ["k"], [("a",), ("b",), ("a", "b")])
    assert gdk.select_groupsum_hash(gp, gk, gs) == (want, True)
    assert gdk.select_groupsum_hash(gp, gk, gs, fused=False) == (want, False)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["one_key", "two_alternating"])
def test_contention_and_carries(gdk, ora, how):
    """All rows on one entry, or on two in turn; an lng column of +-2^62 summed
    alone wraps the low word and carries into negative high words."""
    n = 70_001
    base = make_case(n)
    cols = {c: base[c] for c in ("p0", "p1", "v1", "v2", "v4", "v8")}
    r = np.random.default_rng(31)
    big = r.integers(-(1 << 62), 1 << 62, n).astype(np.int64)
    big[r.random(n) < 0.03] = tnil("lng")
    cols["big"] = ("lng", big)
    cols["k"] = ("int", np.full(n, 123_456, np.int32) if how == "one_key"
                 else np.where(np.arange(n) % 2 == 0, -7, 1 << 30).astype(np.int32))
    want = check_all(gdk, ora, cols, PREDS, ["k"], [("big",), ("v8",), ("v8", ("-", 100, "v4"))])
    assert len(want) == (1, 2)[how == "two_alternating"]
    assert any(abs(g["sums"][0]) > 1 << 64 for g in want)


@pytest.mark.gpu
def test_str_keys(gdk, ora):
    from strheap import build_heap, sample, tail
    n = 2_049
    base = make_case(n)
    r = np.random.default_rng(41)
    # two-byte offsets into a duplicate-eliminated heap: the offsets stand for the strings
    words = [b"word%04d" % i for i in range(60)]
    heap, offs = build_heap(words, 1)
    rel = np.array([offs[w][0] for w in r.integers(0, 60, n)])
    assert rel.max() > 255 and len(heap) < 1 << 16
    cols = {c: base[c] for c in ("p0", "p1", "kb", "v1", "v2", "v4", "v8")}
    cols["ks"] = ("int", rel.astype(np.int32))          # model and oracle: the offsets as integers
    genv = bind(gdk, cols)
    genv["ks"] = gdk.BAT.from_numpy(gdk.TYPE_str, tail(rel, 2), vheap=heap, sorted_=False, revsorted=False, key=False,
                                    nonil=False)
    assert genv["ks"].s.twidth == 2
    want = check_all(gdk, ora, cols, PREDS, ["ks"], SUMS, genv=genv)
    assert len(want) == 60
    check_all(gdk, ora, cols, PREDS, ["kb", "ks"], SUMS, genv=genv)
    # one-byte offsets: the generated lineitem's flags
    dev = gdk.tpch_lineitem(3, 0, n, 20_000)
    host = ora.tpch_lineitem(3, 0, n, 20_000)
    cols = {"shipdate": ("date", host["shipdate"]), "returnflag": ("bte", host["returnflag"].view(np.int8)),
            "linestatus": ("bte", host["linestatus"].view(np.int8)), "q": ("lng", host["quantity"])}
    genv = dict(shipdate=dev["shipdate"], returnflag=dev["returnflag"], linestatus=dev["linestatus"], q=dev["quantity"])
    assert genv["returnflag"].ttype == gdk.TYPE_str and genv["returnflag"].s.twidth == 1
    preds = [("shipdate", int(np.median(host["shipdate"])), "<=")]
    want = check_all(gdk, ora, cols, preds, ["returnflag", "linestatus"], [("q",)], genv=genv)
    assert 2 <= len(want) <= 8
    # a heap of 64 KiB or more may hold one string at several offsets: not applicable
    t, bigheap, _ = sample(r, n, 2)
    assert len(bigheap) >= 1 << 16
    genv = bind(gdk, {c: base[c] for c in ("p0", "p1", "v1", "v2", "v4", "v8")})
    genv["ks"] = gdk.BAT.from_numpy(gdk.TYPE_str, t, vheap=bigheap, sorted_=False, revsorted=False, key=False,
                                    nonil=False)
    errbuf_clean_none(gdk, *bound(genv, PREDS, ["ks"], SUMS))


@pytest.mark.gpu
@pytest.mark.parametrize("why", ["twelve_bytes", "three_keys", "hge_key", "flt_key", "materialised_candidates"])
def test_out_of_scope_answers_cleanly(gdk, why):
    n = 2_049
    genv = bind(gdk, make_case(n))
    keys, s = ["kint"], None
    if why == "twelve_bytes":
        keys = ["klng", "kint"]
    elif why == "three_keys":
        keys = ["kb", "kb3", "ksht"]
    elif why == "hge_key":
        genv["kh"] = gdk.BAT.from_numpy(gdk.TYPE_hge, np.arange(2 * n, dtype=np.uint64) % 3)
        keys = ["kh"]
    elif why == "flt_key":
        genv["kf"] = gdk.BAT.from_numpy(gdk.TYPE_flt, (np.arange(n) % 3).astype(np.float32))
        keys = ["kf"]
    else:
        s = gdk.BAT.from_numpy(gdk.TYPE_oid, np.arange(0, n, 2, dtype=np.uint64))
    gp, gk, gs = bound(genv, PREDS, keys, SUMS)
    errbuf_clean_none(gdk, gp, gk, gs, s)
    if why == "hge_key":
        # the result's keys are 8 bytes: the operators' twin cannot answer either, and says so
        with pytest.raises(gdk.GDKError, match="key column of width 16"):
            gdk.select_groupsum_hash(gp, gk, gs, s)
        with pytest.raises(gdk.GDKError, match="key column of width 16"):
            gdk.select_groupsum_hash(gp, gk, gs, s, fused=False)


@pytest.mark.gpu
def test_narrow_twin_rejects_wider_keys(gdk):
    """mgdk_gsgroup holds one byte per key: the narrow entry's operators refuse an int key instead of reading
    its column back into byte-sized room."""
    genv = bind(gdk, make_case(2_049))
    gp, gk, gs = bound(genv, PREDS, ["kint"], SUMS)
    assert gdk.select_groupsum(gp, gk, gs, fallback=False) is None
    with pytest.raises(gdk.GDKError, match="key column of width 4"):
        gdk.select_groupsum(gp, gk, gs)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["dense_cand", "slices", "aligned_slices", "hseqbase"])
def test_candidates_and_views(gdk, ora, how):
    """A dense candidate list starting mid-column and BATslice views (heaps
    that are not 16-byte aligned) take the guarded loads; a slice starting
    16-byte aligned takes the buffer loads; `first` carries the hseqbase."""
    n = 70_001
    cols = make_case(n)
    keys = ["kb", "kint"]
    if how == "dense_cand":
        check_all(gdk, ora, cols, PREDS, keys, SUMS, s=(123, n - 77))
        return
    if how == "hseqbase":
        want, _ = model(cols, PREDS, keys, SUMS, base=1_000)
        gp, gk, gs = bound(bind(gdk, cols, 1_000), PREDS, keys, SUMS)
        assert gdk.select_groupsum_hash(gp, gk, gs) == (want, True)
        assert ora_chain(ora, bind(ora, cols, 1_000), PREDS, keys, SUMS) == want
        assert min(g["first"] for g in want) >= 1_000
        return
    a, b = (3, n - 5) if how == "slices" else (16, n - 5)
    want, _ = model(cols, PREDS, keys, SUMS, a, b)
    genv = {k: gdk.BATslice(v, a, b) for k, v in bind(gdk, cols).items()}
    assert genv["v8"].hseqbase == a
    gp, gk, gs = bound(genv, PREDS, keys, SUMS)
    assert gdk.select_groupsum_hash(gp, gk, gs) == (want, True)
    assert gdk.select_groupsum_hash(gp, gk, gs, fused=False) == (want, False)
    oenv = bind(ora, {k: (t, v[a:b]) for k, (t, v) in cols.items()}, a)
    assert ora_chain(ora, oenv, PREDS, keys, SUMS) == want


@pytest.mark.gpu
def test_overflow_stays_with_the_operators(gdk, ora):
    big = 1 << 62

    def case(a, b, p, k):
        return {"p": ("int", np.array(p, np.int32)), "k": ("int", np.array(k, np.int32) * 100_000),
                "a": ("lng", np.array(a, np.int64)), "b": ("lng", np.array(b, np.int64))}

    preds, keys = [("p", 0, ">")], ["k"]
    # 100 - col with a surviving col = -(2^63 - 1) leaves lng: declined, and the operators raise
    sums = [(("-", 100, "a"),)]
    cols = case([5, -LNG_MAX, 7, 9], [1] * 4, [1, 1, 1, 1], [1, 2, 1, 2])
    _, live = model(cols, preds, keys, [])
    assert not in_scope(cols, sums, live)
    gp, gk, gs = bound(bind(gdk, cols), preds, keys, sums)
    assert gdk.select_groupsum_hash(gp, gk, gs, fallback=False) is None
    with pytest.raises(ora.OracleError) as oe:
        ora_chain(ora, bind(ora, cols), preds, keys, sums)
    with pytest.raises(gdk.GDKError) as ge:
        gdk.select_groupsum_hash(gp, gk, gs)
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


def lines_touched(mask, width):
    return len(np.unique(np.flatnonzero(mask) * width // 128))


@pytest.mark.gpu
def test_late_materialisation_is_real(gdk):
    """select_groupsum_hash_last_lines counts, for every column after the
    first predicate's -- the 4-byte key included -- the 128-byte lines holding
    a row that passed everything before the column's first use."""
    n = 262_144
    r = np.random.default_rng(11)
    first = np.arange(n, dtype=np.int32)                       # sorted: one contiguous 10 % survives
    cols = {"first": ("int", first), "k": ("sht", r.integers(0, 10, n).astype(np.int16)),
            "g": ("int", r.integers(0, 3, n).astype(np.int32) * 1_000_000),
            "x": ("lng", r.integers(1, 1 << 30, n).astype(np.int64)),
            "y": ("int", r.integers(-100, 100, n).astype(np.int32))}
    lo, hi = n // 3, n // 3 + n // 10
    preds = [("first", lo, hi, True, False, False), ("k", 2, "<=")]
    sums = [("x", "k"), ("y",), ("x", ("-", 100, "y"))]
    want, live = model(cols, preds, ["g"], sums)
    m1 = (first >= lo) & (first < hi)
    assert (live == (m1 & (cols["k"][1] <= 2))).all()
    want_lines = lines_touched(m1, 2) + lines_touched(live, 4) + lines_touched(live, 8) + lines_touched(live, 4)
    gp, gk, gs = bound(bind(gdk, cols), preds, ["g"], sums)
    assert gdk.select_groupsum_hash(gp, gk, gs) == (want, True)
    got = gdk.select_groupsum_hash_last_lines()
    assert got == want_lines
    assert got < (2 + 4 + 8 + 4) * n // 128 // 5               # far below reading the columns whole
