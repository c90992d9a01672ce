"""Host-side mirror of the MAL bindings that sit above the GDK operators.

The reference keeps these bindings unchanged (monetdb5/modules/kernel/
algebra.c, aggr.c, group.c, monetdb5/modules/mal/batcalc.c); they only
normalise arguments and call the BAT* functions.  This module restates the
argument normalisation so that MAL-level known-answer fixtures can be
replayed against any GDK implementation (the HIP product or the oracle):
`gdk` is a module exposing BATselect / BATthetaselect / BATproject / ...
"""


def alg_select_args(low, high, li, hi, anti, unknown, is_nil):
    """ALGselect2nil argument rewrite (monetdb5/modules/kernel/algebra.c:260-316).

    Returns (low, high, li, hi, anti) to pass to BATselect with
    nil_matches=False.  `high` None means "th == NULL" (point select);
    `is_nil(v)` tells whether a value is the type's nil.
    """
    nanti, nli, nhi = anti, li, hi
    if not nanti and unknown:
        if nli and is_nil(low):
            low = high
            nli = False
        if nhi and is_nil(high):
            high = low
            nhi = False
        if low == high and is_nil(high):
            nanti = True
        return low, high, nli, nhi, nanti, False
    if not unknown:
        if nli and nhi and is_nil(low) and is_nil(high):
            # special case: equi-select for NIL
            return low, None, nli, nhi, nanti, True
    return low, high, nli, nhi, nanti, False


def batselect_args(low, high, li, hi, anti, unknown=False, nil=None):
    """The (tl, th, li, hi, anti, nil_matches) algebra.select hands to
    BATselect; a None bound stands for the type's nil."""
    is_nil = (lambda v: v is None or v == nil)
    lo, hg, li2, hi2, anti2, point = alg_select_args(low, high, li, hi, anti, unknown, is_nil)
    lo = nil if lo is None else lo
    if point:
        hg = None
    else:
        hg = nil if hg is None else hg
    return lo, hg, li2, hi2, anti2, False


def ALGselect2(gdk, b, s, low, high, li, hi, anti, unknown=False, nil=None):
    """algebra.select(b, s, low, high, li, hi, anti[, unknown])."""
    return gdk.BATselect(b, s, *batselect_args(low, high, li, hi, anti, unknown, nil))


def ALGthetaselect2(gdk, b, s, val, op):
    """algebra.thetaselect(b, s, val, op) (algebra.c:340-363)."""
    return gdk.BATthetaselect(b, s, val, op)


# ---- MAL plans ----------------------------------------------------------------
# A plan is a list of instructions (results, "module.function[:type]", args):
# `results` a tuple of variable names, `args` variable names or constants.  A
# str argument naming a variable -- one of `env`, or a result of an earlier
# instruction -- stands for its value; every other argument is a constant
# (None: the nil of the column's type).  The ":type" suffix is the MAL result
# type, as in `batcalc.*(pa, pb):hge`.

# run_plan's default for the hashed grouped route: DESIGN.md 11.12
HASHED_DEFAULT = True
# run_plan's default for the star rewrite (fuse_star_groupsum): DESIGN.md 11.13
STAR_DEFAULT = True

SELECTS = ("algebra.select", "algebra.thetaselect")
FUSED = ("mgdk.select_sum", "mgdk.select_groupsum")


def _ttype(b):
    s = b.s
    return s.ttype if hasattr(s, "ttype") else s.type


def _split(fn):
    name, _, tp = fn.partition(":")
    return name, tp


def _select_split(fn, args):
    """(column, candidate or None, the remaining arguments) of a select."""
    if fn == "algebra.thetaselect":
        cand = len(args) == 4
    else:
        # (col, lo, hi, li, hi, anti[, unknown]) or (col, s, lo, hi, li, hi,
        # anti[, unknown]): with seven arguments the fourth is `li`, a bool,
        # only in the form without a candidate list
        cand = len(args) == 8 or (len(args) == 7 and not isinstance(args[3], bool))
    if cand:
        return args[0], args[1], tuple(args[2:])
    return args[0], None, tuple(args[1:])


def _pred_call(gdk, b, fn, rest):
    """The BATselect / BATthetaselect arguments after (b, s) of one select."""
    if fn == "algebra.thetaselect":
        val, op = rest
        return (val, op)
    low, high, li, hi, anti = rest[:5]
    unknown = bool(rest[5]) if len(rest) > 5 else False
    tp = _ttype(b)
    # daytime / timestamp are lng-based where a binding's table lacks them
    nil = gdk.NIL[tp] if tp in gdk.NIL else gdk.NIL[gdk.TYPE_lng]
    return batselect_args(low, high, li, hi, anti, unknown, nil)


def _nil_to_none(gdk, v):
    return None if v == gdk.NIL[gdk.TYPE_hge] else v


def _run_one(gdk, ins, env, hashed=False):
    res, fn, args = ins
    name, tp = _split(fn)
    isvar = (lambda a: isinstance(a, str) and a in env)
    val = (lambda a: env[a] if isvar(a) else a)
    if name in SELECTS:
        col, cand, rest = _select_split(name, args)
        b, s = env[col], (env[cand] if cand is not None else None)
        call = _pred_call(gdk, b, name, rest)
        out = gdk.BATthetaselect(b, s, *call) if name == "algebra.thetaselect" else gdk.BATselect(b, s, *call)
    elif name == "algebra.projection":
        out = gdk.BATproject(val(args[0]), val(args[1]))
    elif name == "algebra.projectionpath":
        # BATprojectchain on the product; nested BATprojects where a binding lacks it
        bats = [val(a) for a in args]
        if hasattr(gdk, "BATprojectchain"):
            out = gdk.BATprojectchain(bats)
        else:
            out = bats[0]
            for b in bats[1:]:
                out = gdk.BATproject(out, b)
    elif name in ("group.group", "group.subgroup"):
        b = val(args[0])
        g = val(args[1]) if name == "group.subgroup" else None
        out = gdk.BATgroup(b, None, g)
        for r, o in zip(res, out):
            env[r] = o
        return
    elif name in ("batcalc.+", "batcalc.-") and tp == "lng" and not isvar(args[0]):
        # cst + b / cst - b: the constant is an lng (BATcalccstadd / BATcalccstsub)
        cst, b = args[0], val(args[1])
        if hasattr(gdk, "BATcalc"):
            out = gdk.BATcalc(name[8:], None, b, gdk.TYPE_lng, c1=cst, t1=gdk.TYPE_lng)
        else:
            out = (gdk.BATcalccstadd if name[8:] == "+" else gdk.BATcalccstsub)(cst, gdk.TYPE_lng, b, gdk.TYPE_lng)
    elif name == "aggr.subsum":
        if tp != "hge":
            raise ValueError(f"{fn}: only an hge result is executed here")
        out = gdk.BATgroupsum(val(args[0]), val(args[1]), val(args[2]), gdk.TYPE_hge, True)
    elif name == "aggr.subcount":
        out = gdk.BATgroupcount(val(args[0]), val(args[1]), val(args[2]), False)
    elif name == "aggr.subavg":
        out = gdk.BATgroupavg3(val(args[0]), val(args[1]), val(args[2]), True)
        for r, o in zip(res, out):
            env[r] = o
        return
    elif name == "mgdk.select_groupsum":
        _run_select_groupsum(gdk, ins, env, hashed)
        return
    elif name.startswith("batcalc.") and name[8:] in ("*", "+", "-"):
        if tp != "hge":
            raise ValueError(f"{fn}: only an hge result is executed here")
        b1, b2 = val(args[0]), val(args[1])
        if hasattr(gdk, "BATcalc"):
            out = gdk.BATcalc(name[8:], b1, b2, gdk.TYPE_hge)
        else:
            out = {"*": gdk.BATcalcmul, "+": gdk.BATcalcadd, "-": gdk.BATcalcsub}[name[8:]](b1, b2, gdk.TYPE_hge)
    elif name == "aggr.sum":
        if tp != "hge":
            raise ValueError(f"{fn}: only an hge result is executed here")
        out = _nil_to_none(gdk, gdk.BATsum(gdk.TYPE_hge, val(args[0])))
    elif name == "aggr.count":
        out = int(val(args[0]).count())
    elif name == "mgdk.select_sum":
        _run_select_sum(gdk, ins, env)
        return
    else:
        raise ValueError(f"unknown MAL instruction {fn}")
    env[res[0]] = out


def _run_select_sum(gdk, ins, env):
    """mgdk.select_sum: the fused operator where the binding has one and it
    applies, otherwise the instructions the rewrite replaced."""
    res, _, (spec,) = ins
    if hasattr(gdk, "select_sum"):
        preds = []
        for fn, col, rest in spec["preds"]:
            b = env[col]
            preds.append((b,) + tuple(_pred_call(gdk, b, fn, rest)))
        sums = [(env[a], env[b] if b is not None else None) for a, b in spec["sums"]]
        s = env[spec["s"]] if spec["s"] is not None else None
        r = gdk.select_sum(preds, sums, s, fused=True, fallback=False)
        if r is not None:
            vals, cnt, _ = r
            for name, v in zip(res, vals + [cnt]):
                env[name] = v
            return
    for k in spec["kept"]:
        _run_one(gdk, k, env)


def run_plan(gdk, plan, env=None, fuse=True, hashed=None, star=None):
    """Execute a plan against a GDK binding (monetdb_amd.gdk or the
    oracle's Python module); returns the variables, `env` included.  Executed:
    algebra.select / thetaselect / projection, batcalc.* / + / - into hge,
    aggr.sum into hge, aggr.count, group.group / subgroup, batcalc.+ / - of a
    constant and a BAT into lng, aggr.subsum into hge, aggr.subcount,
    aggr.subavg (three results) and the mgdk.select_sum / mgdk.select_groupsum
    that fuse_select_sum / fuse_select_groupsum put in.  fuse=True (the
    default: the fused operators beat the operators where they were measured,
    DESIGN.md 11.10, 11.11) applies those rewrites first; a plan that is
    already rewritten is left as it is.  hashed: a mgdk.select_groupsum whose
    keys are wider than a byte, or that the narrow operator declined, tries
    the binding's select_groupsum_hash before the kept instructions (None:
    HASHED_DEFAULT, which follows the measurement of DESIGN.md 11.12).  star:
    the grouped rewrite is fuse_star_groupsum, which also takes fragments with
    columns gathered through a join index to the binding's
    select_groupsum_star (None: STAR_DEFAULT); a plan without
    such a column is rewritten and run the same either way.
    algebra.projectionpath is executed as well."""
    hashed = HASHED_DEFAULT if hashed is None else hashed
    star = STAR_DEFAULT if star is None else star
    env = dict(env or {})
    if fuse:
        plan = (fuse_star_groupsum if star else fuse_select_groupsum)(fuse_select_sum(plan))
    for ins in plan:
        _run_one(gdk, ins, env, hashed)
    return env


def fuse_select_sum(plan):
    """Replace every fragment

        c1 := algebra.select(col1 [, s], lo, hi, li, hi, anti) | algebra.thetaselect(col1 [, s], v, op)
        c2 := algebra.select(col2, c1, ...)                     ... up to four
        pa := algebra.projection(ck, a);  pb := algebra.projection(ck, b)
        m  := batcalc.*(pa, pb):hge                             (optional)
        r  := aggr.sum(m | pa):hge                              up to four
        n  := aggr.count(ck)                                    (optional)

    by one instruction ((r..., [n]), "mgdk.select_sum", (spec,)) placed where
    the fragment's last instruction stood; spec holds the predicates, the
    sums, the first candidate list and, under "kept", the instructions it
    replaces.  Nothing is rewritten unless every intermediate -- c1..ck, the
    projections, the products -- is used inside the fragment only."""
    plan = list(plan)
    defs, uses = {}, {}
    for i, (res, fn, args) in enumerate(plan):
        for r in res:
            defs[r] = i
    for i, (res, fn, args) in enumerate(plan):
        if _split(fn)[0] in FUSED:
            continue
        for a in args:
            if isinstance(a, str) and a in defs and defs[a] < i:
                uses.setdefault(a, []).append(i)
    name_of = (lambda i: _split(plan[i][1])[0])
    type_of = (lambda i: _split(plan[i][1])[1])
    replaced = {}                       # last index of a fragment -> (instruction, its indices)
    taken = set()
    for ck, d in defs.items():
        if name_of(d) not in SELECTS or len(plan[d][0]) != 1:
            continue
        users = uses.get(ck, [])
        proj = [i for i in users if name_of(i) == "algebra.projection" and plan[i][2][0] == ck]
        cnts = [i for i in users if name_of(i) == "aggr.count"]
        if not users or set(users) != set(proj) | set(cnts) or len(cnts) > 1:
            continue                     # ck feeds something else (a further select included)
        pvar = {plan[i][0][0]: i for i in proj}
        prods, sums, ok = {}, [], True
        for p, i in pvar.items():
            for u in uses.get(p, []):
                if name_of(u) == "batcalc.*" and type_of(u) == "hge" and all(a in pvar for a in plan[u][2][:2]) \
                        and len(plan[u][2]) == 2:
                    prods[plan[u][0][0]] = u
                elif name_of(u) == "aggr.sum" and type_of(u) == "hge":
                    if u not in sums:
                        sums.append(u)
                else:
                    ok = False
        for m, i in prods.items():
            for u in uses.get(m, []):
                if name_of(u) == "aggr.sum" and type_of(u) == "hge":
                    if u not in sums:
                        sums.append(u)
                else:
                    ok = False
        sums.sort()
        if not ok or len(sums) > 4 or not (sums or cnts):
            continue
        # the select chain behind ck: every link used by the next one only
        chain, c, s = [], ck, None
        while True:
            i = defs[c]
            col, cand, rest = _select_split(name_of(i), plan[i][2])
            chain.append(i)
            if cand is None:
                break
            if cand not in defs or defs[cand] > i:
                s = cand                 # a plan input: the first candidate list
                break
            if name_of(defs[cand]) not in SELECTS or uses.get(cand, []) != [i]:
                ok = False
                break
            c = cand
        chain.reverse()
        if not ok or len(chain) > 4:
            continue
        idx = set(chain) | set(proj) | set(prods.values()) | set(sums) | set(cnts)
        if idx & taken:
            continue
        spec = {"s": s, "preds": [], "sums": [], "kept": [plan[i] for i in sorted(idx)]}
        for i in chain:
            col, cand, rest = _select_split(name_of(i), plan[i][2])
            spec["preds"].append((name_of(i), col, rest))
        for u in sums:
            x = plan[u][2][0]
            if x in prods:
                pa, pb = plan[prods[x]][2][:2]
                spec["sums"].append((plan[pvar[pa]][2][1], plan[pvar[pb]][2][1]))
            else:
                spec["sums"].append((plan[pvar[x]][2][1], None))
        res = tuple(plan[u][0][0] for u in sums) + tuple(plan[i][0][0] for i in cnts)
        taken |= idx
        replaced[max(idx)] = ((res, "mgdk.select_sum", (spec,)), idx)
    out = []
    for i, ins in enumerate(plan):
        if i in replaced:
            out.append(replaced[i][0])
        elif i not in taken:
            out.append(ins)
    return out


# ---- the grouped fragment ------------------------------------------------------

GS_MAXKEYS, GS_MAXSUMS, GS_MAXFACTORS = 2, 6, 3


def _twidth(b):
    s = b.s
    return s.twidth if hasattr(s, "twidth") else s.width


def _run_select_groupsum(gdk, ins, env, hashed=False):
    """mgdk.select_groupsum: the fused operator where the binding has one and
    it applies -- its group results then stand in for the aggr.sub* results and
    for the projections through the extents -- otherwise the instructions the
    rewrite replaced.  The routes in order: select_groupsum where every key is
    one byte wide; where it declines, and for wider keys at once,
    select_groupsum_hash if the binding has it and `hashed` allows it; the
    kept instructions."""
    res, _, (spec,) = ins
    r = None
    if spec.get("vias"):
        _run_select_groupsum_star(gdk, ins, env)
        return
    if hasattr(gdk, "select_groupsum"):
        preds = []
        for fn, col, rest in spec["preds"]:
            b = env[col]
            preds.append((b,) + tuple(_pred_call(gdk, b, fn, rest)))
        keys = [env[k] for k in spec["keys"]]
        sums = [tuple(env[f] if isinstance(f, str) else (f[0], f[1], env[f[2]]) for f in fs)
                for fs in spec["sums"]]
        s = env[spec["s"]] if spec["s"] is not None else None
        if all(_twidth(k) == 1 for k in keys):
            r = gdk.select_groupsum(preds, keys, sums, s, fused=True, fallback=False)
        if r is None and hashed and hasattr(gdk, "select_groupsum_hash"):
            r = gdk.select_groupsum_hash(preds, keys, sums, s, fused=True, fallback=False)
    if r is None:
        for k in spec["kept"]:
            _run_one(gdk, k, env)
        return
    _groupsum_outs(gdk, spec, r[0], env, env)


def _run_select_groupsum_star(gdk, ins, env):
    """A mgdk.select_groupsum whose spec carries `vias` ({route: (dimension
    column, join index)}): the binding's select_groupsum_star where it has one
    and every join index is an oid column, then the kept instructions.  Each
    route gets a descriptor of its own: the dimension column's for the first
    route to it, a view of it for a further one."""
    res, _, (spec,) = ins
    r = None
    vias = spec["vias"]
    if hasattr(gdk, "select_groupsum_star") and all(_ttype(env[v]) == gdk.TYPE_oid for _, v in vias.values()):
        cols, taken = dict(env), set()
        for rid, (d, v) in vias.items():
            cols[rid] = env[d] if d not in taken else gdk.BATslice(env[d], 0, env[d].count())
            taken.add(d)
        preds = []
        for fn, col, rest in spec["preds"]:
            preds.append((cols[col],) + tuple(_pred_call(gdk, cols[col], fn, rest)))
        keys = [cols[k] for k in spec["keys"]]
        sums = [tuple(cols[f] if isinstance(f, str) else (f[0], f[1], cols[f[2]]) for f in fs)
                for fs in spec["sums"]]
        s = env[spec["s"]] if spec["s"] is not None else None
        r = gdk.select_groupsum_star(preds, keys, sums, [(cols[rid], env[v]) for rid, (d, v) in vias.items()], s,
                                     fused=True, fallback=False)
    if r is None:
        for k in spec["kept"]:
            _run_one(gdk, k, env)
        return
    _groupsum_outs(gdk, spec, r[0], env, cols)


def _groupsum_outs(gdk, spec, groups, env, cols):
    """The results of a mgdk.select_groupsum from the fused operator's groups;
    cols: the columns by the names the spec uses."""
    vias = spec.get("vias") or {}
    lng = (lambda vals: gdk.BAT.from_numpy(gdk.TYPE_lng, [gdk.NIL[gdk.TYPE_lng] if v is None else v for v in vals]))
    first = gdk.BAT.from_numpy(gdk.TYPE_oid, [g["first"] for g in groups])
    for out in spec["outs"]:
        kind = out[0]
        if kind == "sum":
            words = [gdk.int_to_hge_words(gdk.NIL[gdk.TYPE_hge] if g["sums"][out[2]] is None else g["sums"][out[2]])
                     for g in groups]
            env[out[1]] = gdk.BAT.from_numpy(gdk.TYPE_hge, [w for lohi in words for w in lohi])
        elif kind == "count":
            env[out[1]] = lng([g["count"] for g in groups])
        elif kind == "avg":
            # BATgroupavg3 of the column from its exact sum: a group without
            # a non-nil value has a nil average, remainder 0 and count 0
            (a, rm, n), j, col = out[1], out[2], out[3]
            tp = _ttype(cols[col])
            trip = [gdk.avg3_of_sum(g["sums"][j], g["nonnil"][j]) if g["nonnil"][j] else (gdk.NIL[tp], 0)
                    for g in groups]
            env[a] = gdk.BAT.from_numpy(tp, [t[0] for t in trip])
            env[rm] = lng([t[1] for t in trip])
            env[n] = lng([g["nonnil"][j] for g in groups])
        elif kind == "first":
            env[out[1]] = first
        elif out[2] in vias:            # "proj" of a gathered column: through its join index
            d, v = vias[out[2]]
            env[out[1]] = gdk.BATproject(gdk.BATproject(first, env[v]), env[d])
        else:                           # "proj": a column at the groups' first rows
            env[out[1]] = gdk.BATproject(first, env[out[2]])


def fuse_select_groupsum(plan):
    """Replace every fragment

        c1 := algebra.select | algebra.thetaselect(col1 [, s], ...) ... c_k     up to four, or none (c_k = s)
        p  := algebra.projection(ck, col)                                        keys and operands
        (g1, e1, h1) := group.group(pk0);  (g, e, h) := group.subgroup(pk1, g1)  the second one optional
        f  := batcalc.+(cst, p):lng | batcalc.-(cst, p):lng                      a factor (or p itself)
        m  := batcalc.*(f | m, f):hge                                            products, nested from the left
        r  := aggr.subsum(p | f | m, g, e):hge                                   up to six sums in all
        n  := aggr.subcount(p, g, e)
        (a, r, n) := aggr.subavg(p, g, e)                                        over a projected column only
        k  := algebra.projection(e, p | ck)                                      keys / first rows of the groups

    by one instruction (results, "mgdk.select_groupsum", (spec,)) placed
    where the fragment's last instruction stood; spec holds the predicates,
    the key and operand columns, what each result is ("outs") and, under
    "kept", the instructions it replaces.  Nothing is rewritten unless every
    candidate list, projection, factor, product, group-id BAT and histogram is
    used inside the fragment only and the final extents feed nothing but the
    aggregates and such projections."""
    return _fuse_groupsum(plan, False)


def fuse_star_groupsum(plan):
    """fuse_select_groupsum for star joins: the same fragment, in which a key,
    an operand or a predicate's column may be gathered through a join index V
    (an oid column of the fact table, checked when the plan runs) from a column
    D of a dimension table, V and D plan inputs:

        t := algebra.projection(c, V);  x := algebra.projection(t, D)      a gathered value, or
        x := algebra.projectionpath(c, V, D)
        p := algebra.select | algebra.thetaselect(x, ...)                  a gathered predicate: x taken from
        c_i := algebra.projection(p, c_{i-1})                              c_{i-1}, no candidate list in the select

    The emitted mgdk.select_groupsum names a gathered column by its route and
    its spec carries "vias": {route: (D, V)}; run_plan takes such a spec to
    the binding's select_groupsum_star, then to the kept instructions.  A plan
    whose first select is on a gathered column without a candidate-list
    variable before it is left as written; a fragment without a gathered
    column is rewritten exactly as fuse_select_groupsum does."""
    return _fuse_groupsum(plan, True)


def _fuse_groupsum(plan, star):
    plan = list(plan)
    defs, uses = {}, {}
    for i, (res, fn, args) in enumerate(plan):
        for r in res:
            defs[r] = i
    for i, (res, fn, args) in enumerate(plan):
        if _split(fn)[0] in FUSED:
            continue
        for a in args:
            if isinstance(a, str) and a in defs and defs[a] < i:
                uses.setdefault(a, []).append(i)
    name_of = (lambda i: _split(plan[i][1])[0])
    type_of = (lambda i: _split(plan[i][1])[1])
    isdef = (lambda a: isinstance(a, str) and a in defs)
    replaced, taken = {}, set()
    for i0 in range(len(plan)):
        if name_of(i0) != "group.group" or len(plan[i0][0]) != 3 or len(plan[i0][2]) != 1:
            continue
        spec_idx = _groupsum_fragment(plan, i0, defs, uses, name_of, type_of, isdef, star)
        if spec_idx is None:
            continue
        res, spec, idx = spec_idx
        if idx & taken:
            continue
        spec["kept"] = [plan[i] for i in sorted(idx)]
        taken |= idx
        replaced[max(idx)] = (res, "mgdk.select_groupsum", (spec,))
    out = []
    for i, ins in enumerate(plan):
        if i in replaced:
            out.append(replaced[i])
        elif i not in taken:
            out.append(ins)
    return out


def _whole_gather(plan, d, name_of, isinput):
    """Instruction d gathers a dimension column for every row of the fact table:
    algebra.projection(V, D) or algebra.projectionpath(V, D) of plan inputs."""
    a = plan[d][2]
    return name_of(d) in ("algebra.projection", "algebra.projectionpath") and len(a) == 2 and isinput(a[0]) \
        and isinput(a[1])


def _groupsum_fragment(plan, i0, defs, uses, name_of, type_of, isdef, star=False):
    """(results, spec without "kept", instruction indices) of the fragment
    around the group.group at i0, or None.  star: gathered columns too."""
    idx = {i0}
    vias, inner_of = {}, {}
    isinput = (lambda a: isinstance(a, str) and not isdef(a))

    def gathered(v, cand):
        """The route of v = D's values at the candidates cand through a join index, or None;
        notes the projection underneath v so that it joins the fragment with v."""
        if not star or not isdef(v):
            return None
        d = defs[v]
        a = plan[d][2]
        if name_of(d) == "algebra.projectionpath" and len(a) == 3 and a[0] == cand and isinput(a[1]) and isinput(a[2]):
            via, dim = a[1], a[2]
        elif name_of(d) == "algebra.projection" and len(a) == 2 and isdef(a[0]) and isinput(a[1]) \
                and name_of(defs[a[0]]) == "algebra.projection" and len(plan[defs[a[0]]][2]) == 2 \
                and plan[defs[a[0]]][2][0] == cand and isinput(plan[defs[a[0]]][2][1]):
            via, dim = plan[defs[a[0]]][2][1], a[1]
            inner_of[d] = defs[a[0]]
        else:
            return None
        rid = "%s->%s" % (via, dim)
        vias[rid] = (dim, via)
        return rid

    def gathered_pred(i):
        """(the select, its route, c_{i-1}) where instruction i is c_i := algebra.projection(p, c_{i-1}) with p a
        select without candidates on a column gathered from c_{i-1}; else None"""
        a = plan[i][2]
        if not star or name_of(i) != "algebra.projection" or len(a) != 2 or not isdef(a[0]) or not isinstance(a[1], str):
            return None
        pi = defs[a[0]]
        if name_of(pi) not in SELECTS or len(plan[pi][0]) != 1:
            return None
        col, cand, rest = _select_split(name_of(pi), plan[pi][2])
        rid = gathered(col, a[1]) if cand is None else None
        return None if rid is None else (pi, rid, a[1])

    keyvars = [plan[i0][2][0]]
    g, e, h = plan[i0][0]
    # the refining subgroup: the only user of g1, with e1 and h1 unused
    sub = [u for u in uses.get(g, []) if name_of(u) == "group.subgroup"]
    if sub:
        u = sub[0]
        if uses.get(g) != [u] or uses.get(e) or uses.get(h) or len(plan[u][2]) != 2 or plan[u][2][1] != g \
                or len(plan[u][0]) != 3:
            return None
        idx.add(u)
        keyvars.append(plan[u][2][0])
        g, e, h = plan[u][0]
        if any(name_of(v) == "group.subgroup" for v in uses.get(g, [])):
            return None                  # three keys
    if uses.get(h):
        return None
    # the keys: projections of one candidate list
    projs = ("algebra.projection", "algebra.projectionpath") if star else ("algebra.projection",)
    if not all(isdef(k) and name_of(defs[k]) in projs for k in keyvars):
        return None
    ck = plan[defs[keyvars[0]]][2][0]
    if star and name_of(defs[keyvars[0]]) == "algebra.projection" and isdef(ck) \
            and name_of(defs[ck]) == "algebra.projection" and gathered_pred(defs[ck]) is None:
        ck = plan[defs[ck]][2][0]        # a key gathered in two steps: the candidates under the join index
    if not isinstance(ck, str):
        return None
    # a fragment projection: algebra.projection(ck, column), the column a plan input
    def proj_col(v):
        rid = gathered(v, ck)
        if rid is not None:
            return rid
        if not isdef(v) or name_of(defs[v]) != "algebra.projection":
            return None
        l, r = plan[defs[v]][2][:2]
        return r if l == ck and isinstance(r, str) and not isdef(r) else None

    def factor(v):
        """col, (op, cst, col), or None"""
        c = proj_col(v)
        if c is not None:
            idx.add(defs[v])
            return c
        if not isdef(v):
            return None
        d = defs[v]
        if name_of(d) in ("batcalc.+", "batcalc.-") and type_of(d) == "lng" and len(plan[d][2]) == 2:
            cst, p = plan[d][2]
            if isinstance(cst, int) and not isinstance(cst, bool) and proj_col(p) is not None:
                idx.update((d, defs[p]))
                return (name_of(d)[8:], cst, proj_col(p))
        return None

    def factors(v):
        f = factor(v)
        if f is not None:
            return [f]
        if not isdef(v):
            return None
        d = defs[v]
        if name_of(d) == "batcalc.*" and type_of(d) == "hge" and len(plan[d][2]) == 2:
            left, right = factors(plan[d][2][0]), factor(plan[d][2][1])
            if left is None or right is None:
                return None
            idx.add(d)
            return left + [right]
        return None

    keys = [proj_col(k) for k in keyvars]
    if None in keys:
        return None
    idx.update(defs[k] for k in keyvars)
    sums, outs, res = [], [], []
    aggrs = sorted(set(uses.get(g, [])))
    for u in aggrs:
        nm, args = name_of(u), plan[u][2]
        if len(args) != 3 or args[1] != g or args[2] != e:
            return None
        if nm == "aggr.subsum" and type_of(u) == "hge" and len(plan[u][0]) == 1:
            fs = factors(args[0])
            if fs is None or len(fs) > GS_MAXFACTORS:
                return None
            fs = tuple(fs)
            if fs not in sums:
                sums.append(fs)
            outs.append(("sum", plan[u][0][0], sums.index(fs)))
        elif nm == "aggr.subcount" and len(plan[u][0]) == 1:
            if proj_col(args[0]) is None:
                return None
            idx.add(defs[args[0]])
            outs.append(("count", plan[u][0][0]))
        elif nm == "aggr.subavg" and len(plan[u][0]) == 3:
            c = proj_col(args[0])
            if c is None:
                return None
            idx.add(defs[args[0]])
            if (c,) not in sums:
                sums.append((c,))
            outs.append(("avg", tuple(plan[u][0]), sums.index((c,)), c))
        else:
            return None
        idx.add(u)
        res.extend(plan[u][0])
    if not aggrs or len(sums) > GS_MAXSUMS:
        return None
    # the extents: the aggregates, and projections of the fragment's own columns
    for u in sorted(set(uses.get(e, []))):
        if u in idx:
            continue
        if name_of(u) != "algebra.projection" or plan[u][2][0] != e or len(plan[u][0]) != 1:
            return None
        x = plan[u][2][1]
        if x == ck:
            outs.append(("first", plan[u][0][0]))
        elif proj_col(x) is not None:
            idx.add(defs[x])
            outs.append(("proj", plan[u][0][0], proj_col(x)))
        else:
            return None
        idx.add(u)
        res.append(plan[u][0][0])
    # the select chain behind ck: every link used by the fragment only
    chain, s = [], None
    if isdef(ck):
        c = ck
        while True:
            i = defs[c]
            gp = gathered_pred(i)
            if gp is not None:
                pi, rid, cand = gp
                x = defs[plan[pi][2][0]]
                chain.append((pi, rid))
                idx.update((i, pi, x))
                if not isdef(cand) or defs[cand] > i:
                    s = cand             # a plan input: the first candidate list
                    break
                if set(uses.get(cand, [])) != {i, inner_of.get(x, x)}:
                    return None
                c = cand
                continue
            if name_of(i) not in SELECTS or len(plan[i][0]) != 1:
                return None
            col, cand, rest = _select_split(name_of(i), plan[i][2])
            chain.append((i, None))
            if cand is None:
                if star and isdef(col) and _whole_gather(plan, defs[col], name_of, isinput):
                    return None          # a first select on a gathered column: left as written
                break
            if not isdef(cand) or defs[cand] > i:
                s = cand                 # a plan input: the first candidate list
                break
            if uses.get(cand, []) != [i]:
                return None
            c = cand
        chain.reverse()
        if len(chain) > 4:
            return None
        idx.update(i for i, _ in chain)
    else:
        s = ck                           # no select: the groups of a plan's candidate list
    # nothing of the fragment but its results may be used outside it
    idx.update(inner_of[i] for i in list(idx) if i in inner_of)
    if len(vias) > 16:
        return None
    inner = set()
    for i in idx:
        inner.update(plan[i][0])
    for v in inner - set(res):
        if any(u not in idx for u in uses.get(v, [])):
            return None
    spec = {"s": s, "preds": [], "keys": keys, "sums": sums, "outs": outs}
    for i, rid in chain:
        col, cand, rest = _select_split(name_of(i), plan[i][2])
        spec["preds"].append((name_of(i), col if rid is None else rid, rest))
    if vias:
        spec["vias"] = vias
    return tuple(res), spec, idx
