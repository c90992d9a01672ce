"""References and cases for gdk.select_groupsum_star (the fused select cascade
+ GROUP BY sums over a star join), shared by test_star_model.py (CPU: the
model against the oracle's operators) and test_select_groupsum_star.py (GPU:
both against the device twin and the fused kernel).

A case: fact columns {name: (type, values)}, the join indexes among them of
type "oid"; dims {dim: dict(hseq=, cols={name: (type, values)})}; routes
{name: (dim, column, via)} -- a predicate, key or factor naming a route is
gathered; preds / keys / sums as test_select_groupsum_hash takes them."""
import functools

import numpy as np

import test_select_groupsum_hash as H

OID_NIL = 1 << 63
NP = dict(H.NP, oid=np.uint64)
tnil = H.tnil


class BadOid(Exception):
    """A live row's oid names no row of the dimension: the operators' error."""


class Case:
    def __init__(self, fact, dims, routes, preds, keys, sums, s=None):
        self.fact, self.dims, self.routes = fact, dims, routes
        self.preds, self.keys, self.sums, self.s = preds, keys, sums, s
        self.n = len(next(iter(fact.values()))[1])


def gathered(case):
    """Every route as a column of the fact table's length: ({route: (type, values)}, {route: bad oids},
    {route: nil oids}); a nil or bad oid yields the type's nil."""
    cols, bad, nil = {}, {}, {}
    for r, (d, c, v) in case.routes.items():
        t, dv = case.dims[d]["cols"][c]
        o = case.fact[v][1]
        isnil = o == np.uint64(OID_NIL)
        idx = o.astype(np.int64) - case.dims[d]["hseq"]
        inr = ~isnil & (idx >= 0) & (idx < len(dv))
        vals = np.full(case.n, tnil(t), NP[t])
        vals[inr] = dv[idx[inr]]
        cols[r], bad[r], nil[r] = (t, vals), ~isnil & ~inr, isnil
    return cols, bad, nil


def pred_mask(cols, p):
    """H.pred_mask, and BATselect's three forms with both bounds nil: (col, nil, nil, True, True, False, True) is
    IS NULL, (col, nil, nil, True, True, True, True) IS NOT NULL, (col, nil, nil, True, True, False) every non-nil."""
    t, v = cols[p[0]]
    if len(p) >= 6 and p[1] == tnil(t) and p[2] == tnil(t):
        isnull = len(p) > 6 and p[6] and not p[5]
        assert isnull or not p[5] or (len(p) > 6 and p[6])
        return v == tnil(t) if isnull else v != tnil(t)
    return H.pred_mask(cols, p)


def uses(case):
    """The columns in the order the fragment uses them: (name, 'pred' index or None)."""
    out = [(p[0], i) for i, p in enumerate(case.preds)]
    out += [(k, None) for k in case.keys]
    out += [(H.factor_parts(f)[2], None) for fs in case.sums for f in fs]
    return out


def model(case):
    """(groups, live, gathers, lines) in plain integers; BadOid where the operators raise.
    gathers: per use, the rows live at that step whose oid is not nil.  lines: per fact
    column (a route: its join index, 8 bytes wide) at its first use, the 128-byte lines that
    hold a row live at that step -- the first predicate's column is read whole and not
    counted, a dimension column is not counted at all."""
    g, bad, nil = gathered(case)
    cols = dict(case.fact, **g)
    lo, hi = (0, case.n) if case.s is None else case.s
    live = np.zeros(case.n, bool)
    live[lo:hi] = True
    gathers = lines = 0
    seen = set()

    def use(name, first_pred=False):
        nonlocal gathers, lines
        if name in case.routes:
            if (bad[name] & live).any():
                raise BadOid(name)
            gathers += int((live & ~nil[name]).sum())
            col, w = case.routes[name][2], 8
        else:
            col, w = name, np.dtype(NP[cols[name][0]]).itemsize
        if col not in seen:
            seen.add(col)
            if not first_pred:
                lines += H.lines_touched(live, w)

    for i, p in enumerate(case.preds):
        use(p[0], i == 0)
        live = live & pred_mask(cols, p)
    for name, i in uses(case):
        if i is None:
            use(name)
    # the grouping and the sums are H.model's, over the rows found live here
    cols["__live"] = ("bte", live.astype(np.int8))
    groups, live2 = H.model(cols, [("__live", 1, "==")], case.keys, case.sums, lo, hi)
    assert (live2 == live).all()
    return groups, live, gathers, lines


def in_scope(case, live):
    return H.in_scope(dict(case.fact, **gathered(case)[0]), case.sums, live)


def bind(mod, case, override=None):
    """The case's BATs for the oracle or the device binding: (env, vias).  env maps fact
    columns and routes to BATs; each route has a descriptor of its own: the dimension
    column's for its first route, a view of it for any further one.  override: {(dim,
    column): BAT} for columns the model holds in another form (str)."""
    mk = mod.BAT.from_numpy if hasattr(mod, "BAT") else mod.Bat.from_array
    env = {k: mk(getattr(mod, "TYPE_" + t), v) for k, (t, v) in case.fact.items()}
    dimbats, vias = {}, []
    for r, (d, c, v) in case.routes.items():
        if (d, c) not in dimbats:
            t, dv = case.dims[d]["cols"][c]
            b = (override or {}).get((d, c))
            dimbats[d, c] = b if b is not None else mk(getattr(mod, "TYPE_" + t), dv, hseqbase=case.dims[d]["hseq"])
            env[r] = dimbats[d, c]
        elif hasattr(mod, "BATslice"):
            env[r] = mod.BATslice(dimbats[d, c], 0, len(case.dims[d]["cols"][c][1]))
            assert env[r].hseqbase == case.dims[d]["hseq"]
        else:
            env[r] = dimbats[d, c]
        vias.append((env[r], env[v]))
    return env, vias


def ora_chain(ora, case, env=None):
    """The fragment through the oracle's operators, literally: two BATprojects per gather, a
    predicate on a gathered column selecting without candidates and going back through the
    previous candidate list."""
    env = env or bind(ora, case)[0]

    def x(c, name):
        if name in case.routes:
            return ora.BATproject(ora.BATproject(c, env[case.routes[name][2]]), env[name])
        return ora.BATproject(c, env[name])

    def sel(b, c, p):
        return ora.BATthetaselect(b, c, p[1], p[2]) if len(p) == 3 else ora.BATselect(b, c, *p[1:7])

    c = None if case.s is None else ora.Bat.dense(case.s[0], case.s[1] - case.s[0])
    for p in case.preds:
        if p[0] not in case.routes:
            c = sel(env[p[0]], c, p)
        elif c is None:
            c = sel(ora.BATproject(env[case.routes[p[0]][2]], env[p[0]]), None, p)
        else:
            c = ora.BATproject(sel(x(c, p[0]), None, p), c)
    k = [x(c, name) for name in case.keys]
    g, e, h = ora.BATgroup(k[0])
    if len(k) > 1:
        g, e, h = ora.BATgroup(k[1], None, g)
    svals, nvals = [], []
    for fs in case.sums:
        t = None
        for f in fs:
            op, cst, col = H.factor_parts(f)
            v = x(c, col)
            if op:
                v = ora.BATcalc(op, None, v, ora.TYPE_lng, c1=cst, t1=ora.TYPE_lng)
            t = v if t is None else ora.BATcalc("*", t, v, ora.TYPE_hge)
        svals.append(ora.BATgroupsum(t, g, e, ora.TYPE_hge, True).values())
        nvals.append(ora.BATgroupcount(t, g, e, True).values())
    cnt = ora.BATgroupcount(k[0], g, e, False).values()
    first = ora.BATproject(e, c).values()
    kv = [ora.BATproject(e, b).values() for b in k]
    out = []
    for i in range(e.count()):
        ss = [int(sv[i]) for sv in svals]
        out.append(dict(first=int(first[i]), keys=tuple(int(b[i]) for b in kv), count=int(cnt[i]),
                        sums=[None if v == H.HGE_NIL else v for v in ss], nonnil=[int(nv[i]) for nv in nvals]))
    return out


def request(case, env, vias, gdk):
    gp, gk, gs = H.bound(env, case.preds, case.keys, case.sums)
    s = None if case.s is None else gdk.BAT.dense(case.s[0], case.s[1] - case.s[0])
    return gp, gk, gs, vias, s


# ---- generated cases ---------------------------------------------------------------------

SIZES = (1, 255, 256, 257, 513, 2_049, 70_001)
DIMS = [(1, 0), (2, 1000), (300, 0), (300, 1000), (70_000, 0), (70_000, 1000)]
ROUTES = {r: ("A", r[2:], "va") for r in ("A.a1", "A.a2", "A.a4", "A.a8", "A.ak")}
ROUTES.update({"B.b4": ("B", "b4", "vb"), "B.b8": ("B", "b8", "vb"), "A2.a4": ("A", "a4", "va2"),
               "A2.ak": ("A", "ak", "va2")})
P0 = ("p0", 3, 17, True, False, False)
# position -> (preds, keys, sums)
FORMS = {
    "first_pred": ([("A.a4", -(1 << 29), 1 << 29, True, False, False), ("p1", 5, "!=")], ["kf"],
                   [("v8",), ("v4", ("-", 100, "v8"))]),
    "first_pred_only": ([("A.a2", 0, ">=")], ["kf", "B.b4"], [("v4",), ("B.b8",)]),
    "later_pred": ([P0, ("A.a2", 1000, "<"), ("p1", 5, "!="), ("B.b4", 3, "!=")], ["kf"], [("v8",), ("A.a1",)]),
    "key0": ([P0], ["A.ak", "kf"], [("v8",), ("v4", "v4")]),
    "key1": ([P0, ("p1", 5, "!=")], ["kf", "B.b4"], [("v8",)]),
    "factors": ([P0], ["kf"], [("A.a1",), ("A.a2",), ("A.a4",), ("A.a8",), ("v4", ("-", 100, "A.a4")),
                               (("+", 7, "A.a1"), "B.b8", "A.a2")]),
    "two_dims": ([P0, ("A.a1", 50, "<")], ["A.ak", "B.b4"], [("A.a8", "v4"), (("-", 1 << 41, "A.a8"), "B.b8"),
                                                                 ("v8",)]),
    "two_routes": ([P0, ("A2.a4", 0, ">")], ["A.ak", "A2.ak"], [("A.a4",), ("A2.a4",), ("A.a4", "A2.a4")]),
}


@functools.lru_cache(maxsize=None)
def make_star(n, dn=300, dhseq=1000, nil_frac=0.02, seed=0):
    """Fact and two dimensions: A of dn rows at hseqbase dhseq, B of min(dn, 7) rows at 0;
    join indexes va, va2 (into A) and vb (into B) with nil oids sprinkled at nil_frac; operand
    values from +-2^40 so that the overflow rule alone never declines a request."""
    r = np.random.default_rng(9100 + n + 7 * dn + seed)
    bn = min(dn, 7)
    A = {"a1": ("bte", r.integers(-100, 100, dn).astype(np.int8)),
         "a2": ("sht", r.integers(-30000, 30000, dn).astype(np.int16)),
         "a4": ("int", r.integers(-(1 << 30), 1 << 30, dn).astype(np.int32)),
         "a8": ("lng", r.integers(-(1 << 40), 1 << 40, dn).astype(np.int64)),
         "ak": ("int", r.choice(np.array([1992, -(1 << 31), 1998, -1, 70_000], np.int32), dn))}
    B = {"b4": ("int", (np.arange(bn) * 1_000_003 - 5).astype(np.int32)),
         "b8": ("lng", r.integers(-(1 << 40), 1 << 40, bn).astype(np.int64))}
    for c in ("a1", "a2", "a4", "a8", "ak"):
        t, v = A[c]
        if dn > 2:
            v[r.random(dn) < 0.03] = tnil(t)
    fact = {"p0": ("int", r.integers(0, 20, n).astype(np.int32)), "p1": ("sht", r.integers(0, 9, n).astype(np.int16)),
            "kf": ("bte", r.choice(np.array([1, 2, -128], np.int8), n)),
            "v4": ("int", r.integers(-(1 << 30), 1 << 30, n).astype(np.int32)),
            "v8": ("lng", r.integers(-(1 << 40), 1 << 40, n).astype(np.int64)),
            "va": ("oid", (r.integers(0, dn, n) + dhseq).astype(np.uint64)),
            "va2": ("oid", (r.integers(0, dn, n) + dhseq).astype(np.uint64)),
            "vb": ("oid", r.integers(0, bn, n).astype(np.uint64))}
    for c in ("p0", "p1", "v4", "v8"):
        t, v = fact[c]
        v[r.random(n) < 0.03] = tnil(t)
    for c in ("va", "va2", "vb"):
        fact[c][1][r.random(n) < nil_frac] = OID_NIL
    return fact, {"A": dict(hseq=dhseq, cols=A), "B": dict(hseq=0, cols=B)}


def star_case(n, form, dn=300, dhseq=1000, s=None, nil_frac=0.02):
    fact, dims = make_star(n, dn, dhseq, nil_frac)
    preds, keys, sums = FORMS[form]
    named = {p[0] for p in preds} | set(keys) | {H.factor_parts(f)[2] for fs in sums for f in fs}
    return Case(fact, dims, {r: v for r, v in ROUTES.items() if r in named}, preds, keys, sums, s)


def generated_cases():
    """id -> Case: every form at every size; every dimension size and hseqbase; a dense
    candidate list starting mid-column."""
    out = {}
    for n in SIZES:
        for form in FORMS:
            out["%s-%d" % (form, n)] = functools.partial(star_case, n, form)
    for dn, dh in DIMS:
        # no nil oids into a dimension of one row: the reference's BATproject marks what it takes
        # from a one-row column as constant, and BATgroup then believes it
        for form in ("two_dims", "first_pred", "factors"):
            out["%s-dim%d@%d" % (form, dn, dh)] = functools.partial(star_case, 2_049, form, dn, dh,
                                                                     nil_frac=0.0 if dn == 1 else 0.02)
    for form in ("first_pred", "later_pred", "key0", "factors"):
        out["%s-dense_s" % form] = functools.partial(star_case, 70_001, form, s=(123, 70_001 - 77))
    return out


def merge_case():
    """70 001 rows, 200 groups keyed by a gathered column (199 values and the nil key of the nil
    oids), every workgroup meeting most of them."""
    n, dn = 70_001, 5_000
    r = np.random.default_rng(77)
    keyvals = (r.permutation(199) * 37 - 3000).astype(np.int32)
    dims = {"A": dict(hseq=1000, cols={"ak": ("int", keyvals[np.arange(dn) % 199]),
                                       "a8": ("lng", r.integers(-(1 << 40), 1 << 40, dn).astype(np.int64))})}
    va = (r.integers(0, dn, n) + 1000).astype(np.uint64)
    va[r.random(n) < 0.02] = OID_NIL
    fact = {"p0": ("int", H.filtered_p0(n)), "va": ("oid", va),
            "v4": ("int", r.integers(-(1 << 30), 1 << 30, n).astype(np.int32))}
    routes = {"A.ak": ("A", "ak", "va"), "A.a8": ("A", "a8", "va")}
    return Case(fact, dims, routes, [P0], ["A.ak"], [("v4",), ("A.a8",), ("v4", ("-", 100, "A.a8"))])


def bad_oid_case(where, removed, kind="beyond"):
    """One oid outside the dimension (beyond its end, or below its hseqbase) on row 300 of 2 049, used by
    the given position; removed: an earlier predicate removes that row."""
    base = star_case(2_049, {"pred": "later_pred", "key": "key0", "factor": "factors"}[where], nil_frac=0.0)
    fact = {k: (t, v.copy()) for k, (t, v) in base.fact.items()}
    fact["va"][1][300] = 1000 + 300 if kind == "beyond" else 999
    fact["p0"][1][300] = 0 if removed else 10
    fact["p1"][1][300] = 1
    return Case(fact, base.dims, base.routes, base.preds, base.keys, base.sums)


def overflow_case(reached):
    """A dimension row holding 2^62 under cst + col with cst = 2^62: leaves lng where a survivor
    reaches it, decides nothing where none does."""
    n = 600
    r = np.random.default_rng(5)
    a8 = r.integers(-1000, 1000, 10).astype(np.int64)
    a8[7] = 1 << 62
    va = r.integers(0, 7, n).astype(np.uint64)
    p0 = np.full(n, 10, np.int32)
    va[100], p0[100] = 7, (10 if reached else 0)
    fact = {"p0": ("int", p0), "va": ("oid", va), "kf": ("bte", (np.arange(n) % 3).astype(np.int8))}
    dims = {"A": dict(hseq=0, cols={"a8": ("lng", a8)})}
    return Case(fact, dims, {"A.a8": ("A", "a8", "va")}, [P0], ["kf"], [(("+", 1 << 62, "A.a8"),), ("A.a8",)])


NIL4 = tnil("int")
NIL_FORMS = {"isnull": ("A.a4", NIL4, NIL4, True, True, False, True),
             "notnull": ("A.a4", NIL4, NIL4, True, True, True, True),
             "range_nil": ("A.a4", NIL4, NIL4, True, True, False)}


def null_fk_case(form, first, bad=False):
    """A filter on a NULL foreign key: a nil-bounded predicate on a gathered column whose dimension holds no nil
    (and says so) while 2 % of the join index are nil oids; first: as the first predicate, else after one on a
    fact column.  bad: row 300, live there, holds an oid beyond the dimension."""
    n, dn = 2_049, 300
    r = np.random.default_rng(61)
    a4 = r.integers(1, 1 << 30, dn).astype(np.int32)
    va = (r.integers(0, dn, n) + 1000).astype(np.uint64)
    va[r.random(n) < 0.02] = OID_NIL
    p0 = H.filtered_p0(n).copy()
    p0[300] = 10
    if bad:
        va[300] = 1000 + dn
    fact = {"p0": ("int", p0), "va": ("oid", va), "kf": ("bte", (np.arange(n) % 3).astype(np.int8)),
            "v8": ("lng", r.integers(-(1 << 40), 1 << 40, n).astype(np.int64))}
    dims = {"A": dict(hseq=1000, cols={"a4": ("int", a4)})}
    preds = [NIL_FORMS[form]] if first else [P0, NIL_FORMS[form]]
    return Case(fact, dims, {"A.a4": ("A", "a4", "va")}, preds, ["kf"], [("v8",), ("A.a4",)])


def empty_after_gather_case(bad):
    """A predicate that no row can pass (lo > hi) after a gathered one: the operators still project for the
    gathered predicate, and raise where a live row's oid is beyond the dimension."""
    case = null_fk_case("notnull", first=False, bad=bad)
    return Case(case.fact, case.dims, case.routes, case.preds + [("p0", 9, 3, True, True, False)], case.keys,
                case.sums)
