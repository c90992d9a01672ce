"""Integer BATsum / BATgroupsum (gdk_aggr.c:900 / :1018 over dosum :708,
AGGR_SUM :429-705) with inputs whose running sums come close to the result
type's range, touch it and leave it.

The arbiter is `sum_model`, a Python-integer restatement of dosum that calls
nothing of the oracle: rows in candidate order; a row whose group id is nil or
outside [min, min + ngrp) is ignored; a group's first value sets its sum to 0
(a nil before it is forgotten); without skip_nils a nil makes the sum nil, and
with one group (or plain BATsum) ends the adding; a nil group skips its adds;
after every add a sum outside [-max, max] of the result type is OVERFLOW.

Inputs.  `_seq` builds one group's rows from the running sums it wants: a
zigzag between 0 and T (the largest multiple of the step `big` below max - 40)
plus noise in [-8, 8], so every running sum stays in range while count * max|v|
exceeds max -- the gate of the ordered decision opens and the decision has to
answer "no".  A plant inserts the pair (+x, -x) after p rows, where the running
sum stands at T: x takes it exactly to max ("exact", legal) or to max + 1
("over", the error); the final sum is the unplanted one.  sign = -1 mirrors the
group, for -max and -max - 1.  Where count * max|v| cannot reach max (bte into
lng ...) nothing can be planted: such calls only check values, and
`_sweep_is_honest` (run by the CPU tests test_oracle_sum / test_oracle_groupsum
over the model's answers) asserts that none of them overflows instead of the
ratios.  sht into int would need a zigzag of 131 077 rows: BATsum plants on a
plain ramp of 65 538 maximal values there, the grouped calls check values.

Type pairs: the entry points accept every integer source with every integer
result, narrower results included (int_type(b->ttype) && int_type(tp) in
aggr.hip; a narrower result just overflows sooner), so PAIRS is all 25.  A
source or result that is no integer is refused with the reference's message.
"""
import numpy as np
import pytest

from helpers import rng
from test_products import OID_NIL, _column, _dense, _err, _imax, _inil, _is_dev, _oids, _result

OVERFLOW = "OVERFLOW"
TYPES = ["bte", "sht", "int", "lng", "hge"]
PAIRS = [(tn, tp) for tn in TYPES for tp in TYPES]
# the pairs that get every grouped configuration; the others get two
HEAVY = [("bte", "bte"), ("lng", "lng"), ("hge", "hge"), ("hge", "lng"), ("bte", "sht")]


# ---- the model --------------------------------------------------------------


def sum_model(vals, gids, mn, ngrp, skip, tp, nil_if_empty=True):
    """vals: the candidate rows (None: nil).  gids None: BATsum, the result or
    None (nil); else BATgroupsum over the groups [mn, mn + ngrp), a list.
    OVERFLOW where the reference raises."""
    mx = _imax(tp)
    plain = gids is None
    ng = 1 if plain else ngrp
    acc, seen, nil = [0] * ng, [False] * ng, [False] * ng
    for i, v in enumerate(vals):
        k = 0
        if not plain:
            g = gids[i]
            if g is None or g < mn or g >= mn + ngrp:
                continue
            k = g - mn
        if v is None:
            if not skip:
                nil[k] = True
                if ng == 1:
                    break
            continue
        if not seen[k]:
            seen[k], nil[k], acc[k] = True, False, 0
        if nil[k]:
            continue
        z = acc[k] + v
        if z < -mx or z > mx:
            return OVERFLOW
        acc[k] = z
    if plain:
        if nil[0]:
            return None
        return acc[0] if seen[0] else (None if nil_if_empty else 0)
    return [acc[k] if seen[k] and not nil[k] else None for k in range(ng)]


def test_model_rules():
    m62 = 1 << 62
    # transient overflow inside a group; values after a group's nil; one group
    assert sum_model([m62, 5, m62, 1, -m62, 2], [0, 1, 0, 1, 0, 1], 0, 2, True, "lng") == OVERFLOW
    assert sum_model([1, 5, None, m62, m62, m62], [0, 1, 0, 0, 0, 0], 0, 2, False, "lng") == [None, 5]
    assert sum_model([1, None, m62, m62, m62], [0] * 5, 0, 1, False, "lng") == [None]
    assert sum_model([1, None, m62, m62, m62], [0] * 5, 0, 1, True, "lng") == OVERFLOW
    # a nil before the first value: forgotten with several groups, final with one
    assert sum_model([None, 4, 7], [0, 0, 1], 0, 2, False, "lng") == [4, 7]
    assert sum_model([None, 4], [0, 0], 0, 1, False, "lng") == [None]
    # ids that do not count, exactly max, the nil value
    assert sum_model([m62, m62, 3], [None, 9, 1], 1, 2, True, "lng") == [3, None]
    assert sum_model([127], None, 0, 0, True, "bte") == 127
    assert sum_model([127, 1], None, 0, 0, True, "bte") == OVERFLOW
    assert sum_model([-127, -1], None, 0, 0, True, "bte") == OVERFLOW
    assert sum_model([1 << 126] * 4, None, 0, 0, True, "hge") == OVERFLOW
    assert sum_model([], None, 0, 0, True, "int") is None and sum_model([], None, 0, 0, True, "int", False) == 0


# ---- one group's rows -------------------------------------------------------


def _shape(tn, tp):
    """(big, q): the zigzag's step and the rows it takes from 0 to its top"""
    S, M = _imax(tn), _imax(tp)
    big = M - 40 if S >= M else S // 2
    return big, (M - 40) // big


def _feasible(tn, tp, L):
    """can a group of L rows be taken to the result type's maximum?"""
    return L >= _shape(tn, tp)[1] + 1


def _seq(r, tn, tp, L, plant=None, p=None, sign=1, nil_at=None):
    """L rows (L + 2 with a plant after p rows, p >= q; + 1 with a nil
    inserted in front of row nil_at of the result)"""
    big, q = _shape(tn, tp)
    M = _imax(tp)
    lead = (p - q) % (2 * q) if plant else 0
    assert not plant or q <= p <= L, (p, q, L)
    w = r.integers(-8, 9, L + 1)
    P = [0] * (L + 1)
    for i in range(1, L + 1):
        t = (i - lead) % (2 * q) if i > lead else 0
        P[i] = big * (q - abs(t - q)) + int(w[i])
    v = [sign * (P[i] - P[i - 1]) for i in range(1, L + 1)]
    if plant:
        x = sign * ((M if plant == "exact" else M + 1) - P[p])
        v[p:p] = [x, -x]
    if nil_at is not None:
        v.insert(nil_at, None)
    return v


def _gate(tn, tp, c, open_):
    """c rows of one size: count * bound just below the maximum (the gate
    stays shut), or just above it with the last two rows negative (open, no
    overflow); None where the source type cannot hold such values"""
    S, M = _imax(tn), _imax(tp)
    v = M // c + 2 if open_ else M // c - 4
    if v > S or v < 1 or c * c >= M:
        return None
    return [v] * (c - 2) + ([-v, -v] if open_ else [v, v])


def test_seq_stays_in_range():
    """unplanted rows never overflow although count * max|v| exceeds the
    maximum; "exact" is legal, "over" is not, on both sides"""
    r = rng(1701)
    for tn, tp in PAIRS:
        S, M = _imax(tn), _imax(tp)
        q = _shape(tn, tp)[1]
        L = min(q + 40, 3000)
        for sign in (1, -1):
            rows = _seq(r, tn, tp, L, sign=sign)
            assert all(abs(x) <= S for x in rows)
            assert sum_model(rows, None, 0, 0, True, tp) == sum(rows)
            if not _feasible(tn, tp, L):
                assert L * S <= M or q > 3000
                continue
            assert L * max(abs(x) for x in rows) > M, (tn, tp)
            for p in (q, q + 2 * q * ((L - q) // (4 * q)), L - (L - q) % (2 * q)):
                ex = _seq(r, tn, tp, L, "exact", p, sign)
                ov = _seq(r, tn, tp, L, "over", p, sign)
                assert all(abs(x) <= S for x in ex + ov), (tn, tp, p)
                assert sum_model(ex, None, 0, 0, True, tp) == sum(ex), (tn, tp, p, sign)
                assert sum_model(ov, None, 0, 0, True, tp) == OVERFLOW, (tn, tp, p, sign)
                assert abs(sum(ov)) <= M
    for tn, tp in PAIRS:
        for open_ in (False, True):
            rows = _gate(tn, tp, 7, open_)
            if rows is not None:
                assert sum_model(rows, None, 0, 0, True, tp) == sum(rows)
                assert (7 * (max(rows) + 2) > _imax(tp)) == open_


# ---- both libraries behind one face -----------------------------------------


def _bat(mod, tn, vals, hseq=0):
    tp = getattr(mod, "TYPE_" + tn)
    arr = _column(vals, tn)
    nonil = all(x is not None for x in vals)
    if _is_dev(mod):
        return mod.BAT.from_numpy(tp, arr, hseqbase=hseq, sorted_=False, revsorted=False, key=False, nonil=nonil)
    return mod.Bat.from_array(tp, arr, hseqbase=hseq, nonil=nonil)


def _cand(mod, rows, sform, huge, hseq):
    """the candidate rows inside a column that also holds rows which must not
    count: (column values, s).  sform: None, ("slice", k) -- k rows before the
    slice -- or "oids" -- a candidate list that leaves rows out"""
    if sform is None:
        return rows, None
    if sform == "oids":
        col, pos = [], []
        for i, x in enumerate(rows):
            if i % 97 == 0 or i == len(rows) - 1:
                col.append(huge if i % 2 else -huge)
            pos.append(len(col))
            col.append(x)
        col.append(huge)
        return col, _oids(mod, [hseq + p for p in pos], sorted_=True, key=True, nonil=True)
    k = sform[1]
    return [huge, -huge, huge][:k] + rows + [huge], _dense(mod, hseq + k, len(rows), 0)


def _first(rows, sform):
    """position in the column of the first candidate"""
    return 0 if sform is None else 1 if sform == "oids" else sform[1]


class SumCase:
    def __init__(self, name, tn, rows, skip=True, ne=True, sform=None, hseq=0):
        self.name, self.tn, self.rows, self.skip, self.ne, self.sform, self.hseq = name, tn, rows, skip, ne, sform, hseq

    def model(self, tp):
        return sum_model(self.rows, None, 0, 0, self.skip, tp, self.ne)

    def call(self, mod, tp):
        col, s = _cand(mod, self.rows, self.sform, _imax(self.tn), self.hseq)
        b = _bat(mod, self.tn, col, self.hseq)
        return mod.BATsum(getattr(mod, "TYPE_" + tp), b, s, self.skip, self.ne)


class GroupCase:
    """rows and ids of the candidates; e: (hseqbase, count) or None"""

    def __init__(self, name, tn, rows, ids, gsorted, skip=True, e=None, sform=None, hseq=0, img8=False):
        self.name, self.tn, self.rows, self.ids, self.gsorted = name, tn, rows, ids, gsorted
        self.skip, self.e, self.sform, self.hseq, self.img8 = skip, e, sform, hseq, img8

    def range(self):
        if self.e is not None:
            return self.e
        ids = [g for g in self.ids if g is not None]
        return (min(ids), max(ids) - min(ids) + 1) if ids else (0, 0)

    def model(self, tp):
        mn, ng = self.range()
        return sum_model(self.rows, self.ids, mn, ng, self.skip, tp)

    def call(self, mod, tp):
        col, s = _cand(mod, self.rows, self.sform, _imax(self.tn), self.hseq)
        b = _bat(mod, self.tn, col, self.hseq)
        ghseq = self.hseq + _first(self.rows, self.sform)
        ids = [OID_NIL if x is None else x for x in self.ids]
        key = self.gsorted and len(set(ids)) == len(ids)
        g = _oids(mod, ids, ghseq, self.gsorted, key, None not in self.ids)
        if self.img8 and _is_dev(mod):
            # the 1-byte id image BATgroup keeps with its result (<= 255 groups):
            # ids in order of first appearance, which is how the cases number them
            g, _, _ = mod.BATgroup(g, want_histo=False)
            assert np.array_equal(g.to_numpy(), np.asarray(ids, np.uint64))
            g.s.hseqbase = ghseq
        e = _dense(mod, 0, self.e[1], self.e[0]) if self.e is not None else None
        return _result(mod, mod.BATgroupsum(b, g, e, getattr(mod, "TYPE_" + tp), self.skip, s))


_MSG = {}


def _overflow_text(ora):
    """the oracle's message, which the device's has to equal"""
    if not _MSG:
        with pytest.raises(ora.OracleError) as e1:
            ora.BATsum(ora.TYPE_bte, _bat(ora, "bte", [127, 1]))
        with pytest.raises(ora.OracleError) as e2:
            ora.BATgroupsum(_bat(ora, "bte", [127, 1]), _oids(ora, [0, 0]), None, ora.TYPE_bte)
        assert str(e1.value) == str(e2.value) and "22003!overflow in sum aggregate." in str(e1.value)
        _MSG["t"] = str(e1.value)
    return _MSG["t"]


def _check(mod, ora, case, tp, want, tally):
    """mod's answer to one case against the model's"""
    what = (case.name, case.tn, tp, case.skip, "device" if _is_dev(mod) else "oracle")
    tally["calls"] += 1
    if want == OVERFLOW:
        tally["overflow"] += 1
        with pytest.raises(_err(mod)) as ei:
            case.call(mod, tp)
        assert str(ei.value) == _overflow_text(ora), what
        return
    got = case.call(mod, tp)
    nil = _inil(tp)
    if isinstance(case, SumCase):
        tally["groups"] += 1
        tally["nonnil"] += want is not None
        assert int(got) == (nil if want is None else want), what
        return
    mn, ng = case.range()
    assert (got["hseq"], got["count"]) == (mn, ng), what
    w = [nil if x is None else x for x in want]
    g = [int(x) for x in got["vals"]]
    bad = [i for i in range(ng) if w[i] != g[i]]
    assert not bad, (what, bad[:8], [g[i] for i in bad[:8]], [w[i] for i in bad[:8]])
    anynil = None in want
    assert (got["nil"], got["nonil"]) == (anynil, not anynil), what
    tally["groups"] += ng
    tally["nonnil"] += sum(x is not None for x in want)


def _tally():
    return {"calls": 0, "overflow": 0, "groups": 0, "nonnil": 0}


def _sweep_is_honest(t, feasible, what):
    """at least half of the calls return values, three quarters of their
    groups non-nil, and at least a quarter of the calls overflow; where the
    type pair cannot overflow at this size, no call does"""
    if feasible is None:
        return
    if not feasible:
        assert t["overflow"] == 0, what
        return
    assert 2 * (t["calls"] - t["overflow"]) >= t["calls"], (what, t)
    assert 4 * t["overflow"] >= t["calls"], (what, t)
    assert 4 * t["nonnil"] >= 3 * t["groups"], (what, t)


# ---- BATsum -----------------------------------------------------------------

SUM_N = [1, 255, 256, 257, 768, 769, 4099, 70001]
SFORMS = [None, "oids", ("slice", 1), ("slice", 3)]


def _positions(n, q, L):
    """plants after p rows, in terms of k_sum_ordered's chunks of
    ceil(n / 256) rows per lane: the pair (p, p + 1) first in a lane's chunk,
    in its middle, last in it and across the border to the next lane's"""
    ch = (n + 255) // 256
    out = []
    for lane in (1, 100, 254, q // ch + 1, q // ch + 2):
        a = lane * ch
        for p in (a, a + ch // 2, a + ch - 2, a + ch - 1):
            # the zigzag stands at its top after p = q, 3q, 5q ... rows plus the
            # lead _seq puts in front: any p >= q will do
            if max(q, 1) <= p <= L and p not in out:
                out.append(p)
    return out


def _sum_cases(tn, tp, n, seed=1710):
    """the BATsum calls of one type pair and size"""
    r = rng(seed + n)
    S, M = _imax(tn), _imax(tp)
    q = _shape(tn, tp)[1]
    k = 0

    def form():
        nonlocal k
        k += 1
        return {"sform": SFORMS[k % 4], "hseq": (0, 5)[k // 4 % 2]}

    if n == 1:
        yield SumCase("max", tn, [min(S, M)])
        yield SumCase("-max", tn, [-min(S, M)], **form())
        yield SumCase("nil", tn, [None], False, **form())
        yield SumCase("nil skipped", tn, [None], True, **form())
        yield SumCase("nil skipped, 0", tn, [None], True, False, **form())
        yield SumCase("empty, 0", tn, [], True, False)
        if S > M:
            yield SumCase("max + 1", tn, [M + 1], **form())
            yield SumCase("-max - 1", tn, [-M - 1], **form())
            yield SumCase("nil then max + 1", tn, [None, M + 1], False, **form())
        return
    for sign in (1, -1):
        yield SumCase("base %d" % sign, tn, _seq(r, tn, tp, n, sign=sign), **form())
    for open_ in (False, True):
        rows = _gate(tn, tp, min(n, 7 if M < 1 << 15 else 50), open_)
        if rows is not None:
            yield SumCase("gate open %d" % open_, tn, rows, **form())
    if not _feasible(tn, tp, n - 2):
        if _ramp_fits(tn, tp, n):
            # the zigzag needs more rows than n, a plain ramp of the source type's
            # maximum does not (sht into int at 70001 rows): c rows of it stay in
            # range, then the pair, then +-S to the end
            c = M // S
            for sign in (1, -1):
                for plant, x in (("ramp", 0), ("exact", M - c * S), ("over", M + 1 - c * S)):
                    rows = [S] * c + [x, -x] + [-S, S] * ((n - c - 2) // 2) + [0] * ((n - c) % 2)
                    yield SumCase("%s %d" % (plant, sign), tn, [sign * v for v in rows], **form())
        return
    pos = _positions(n, q, n - 3)
    if n > 5000:
        pos = pos[1::5] or pos[:1]
    for j, p in enumerate(pos):
        for sign in (1, -1):
            yield SumCase("exact %d @%d" % (sign, p), tn, _seq(r, tn, tp, n - 2, "exact", p, sign), **form())
            yield SumCase("over %d @%d" % (sign, p), tn, _seq(r, tn, tp, n - 2, "over", p, sign), **form())
        if j % 2 == 0 and n > 5000:
            continue
        sign = 1 if j % 2 else -1
        # d) the nil after the planted pair: the error; in front of it: nil
        yield SumCase("over, nil @%d" % p, tn, _seq(r, tn, tp, n - 3, "over", p, sign, p + 2), False, **form())
        yield SumCase("nil, over @%d" % p, tn, _seq(r, tn, tp, n - 3, "over", p, sign, p), False, **form())
        yield SumCase("nils skipped, exact @%d" % p, tn, _seq(r, tn, tp, n - 3, "exact", p, sign, p + 1), **form())
        yield SumCase("nils skipped, over @%d" % p, tn, _seq(r, tn, tp, n - 3, "over", p, sign, p), **form())
    if tn == "hge" and tp == "hge" and n >= 768:
        ch = (n + 255) // 256
        small = [int(x) for x in r.integers(-9, 10, n)]
        # c) a total that wraps to an in-range value
        rows = list(small)
        for i in (0, ch, 2 * ch, 3 * ch):
            rows[i] = 1 << 126
        yield SumCase("4 x 2^126", tn, rows)
        # a lane's own chunk adds up to 2^127 while every running sum of the
        # column is in range: the lanes before it left the sum at -1.5 * 2^126
        rows = list(small)
        rows[0] = -(1 << 126) - (1 << 125)
        rows[5 * ch], rows[5 * ch + 1] = 1 << 126, 1 << 126
        yield SumCase("chunk sum 2^127, in range", tn, rows)
        # the running sum passes 2^127 inside one lane's chunk / only across two
        rows = list(small)
        rows[7 * ch], rows[7 * ch + 1], rows[7 * ch + 2] = 1 << 126, (1 << 126) + 50, -(1 << 126)
        yield SumCase("2^127 inside a chunk", tn, rows)
        rows = list(small)
        rows[8 * ch - 1], rows[8 * ch], rows[8 * ch + 1] = 1 << 126, (1 << 126) + 50, -(1 << 126)
        yield SumCase("2^127 across chunks", tn, rows)
        rows = list(small)
        rows[8 * ch - 1], rows[8 * ch], rows[8 * ch + 1] = -(1 << 126), -(1 << 126) - 50, 1 << 126
        yield SumCase("-2^127 across chunks", tn, rows)


def _ramp_fits(tn, tp, n):
    S, M = _imax(tn), _imax(tp)
    return S < M and n >= M // S + 4


def _sum_feasible(tn, tp, n):
    """can a BATsum call of n rows overflow?  None: n = 1, no ratios"""
    return None if n == 1 else _feasible(tn, tp, n - 2) or _ramp_fits(tn, tp, n)


def _run_cases(mod, ora, cases, tp, feasible, what):
    t = _tally()
    for c in cases:
        _check(mod, ora, c, tp, c.model(tp), t)
    _sweep_is_honest(t, feasible, what)
    return t


@pytest.mark.parametrize("n", SUM_N)
@pytest.mark.parametrize("tn,tp", PAIRS)
def test_oracle_sum(ora, tn, tp, n):
    """ora_sum against the model, and the sweep's ratios"""
    _run_cases(ora, ora, _sum_cases(tn, tp, n), tp, _sum_feasible(tn, tp, n), (tn, tp, n))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SUM_N)
@pytest.mark.parametrize("tn,tp", PAIRS)
def test_gpu_sum(gdk, ora, tn, tp, n):
    """k_sum / k_sum_fin, and behind the gate k_sum_ordered: one row per lane
    (n <= 256), chunks of 2 .. 4 rows (257, 768, 769), of 17 (4099) and of 274
    with several workgroups of k_sum (70001)"""
    _run_cases(gdk, ora, _sum_cases(tn, tp, n), tp, _sum_feasible(tn, tp, n), (tn, tp, n))


# ---- BATgroupsum ------------------------------------------------------------

# name: (groups, layout, rows); layout "u": unsorted ids, "s": sorted, "r": one row per group
CONFIGS = {
    "k1": (1, "u", 20000), "k2": (2, "u", 20000), "k4": (4, "u", 20000), "k5": (5, "u", 20000),
    "k8": (8, "u", 20000), "k2-img8": (2, "u", 20000), "k8-img8": (8, "u", 20000),
    "s9": (9, "s", 20000), "s300": (300, "s", 20000), "rows": (20000, "r", 20000),
    "u300": (300, "u", 20000), "u20000": (20000, "u", 40000),
}
LIGHT_CONFIGS = ["k2", "s9"]
GROUP_PARAMS = [(tn, tp, c) for tn, tp in PAIRS for c in CONFIGS if (tn, tp) in HEAVY or c in LIGHT_CONFIGS]


def _sizes(r, n, ng):
    """group sizes: about n / ng each, at least 1"""
    if ng == n:
        return [1] * ng
    base = n // ng
    return [max(1, base + int(d)) for d in r.integers(-(base // 4), base // 4 + 1, ng)]


class Layout:
    """where the groups' rows go in the candidate sequence, each group's rows
    keeping their order.  "u": the groups' rows shuffled together, the groups
    numbered in order of first appearance (as BATgroup numbers them); else one
    group after the other"""

    def __init__(self, r, lens, layout):
        gid = np.repeat(np.arange(len(lens)), lens)
        if layout == "u":
            gid = r.permutation(gid)
            first = np.full(len(lens), len(gid), np.int64)
            np.minimum.at(first, gid, np.arange(len(gid)))
            rank = np.empty(len(lens), np.int64)
            rank[np.argsort(first, kind="stable")] = np.arange(len(lens))
            gid = rank[gid]
            lens = [int(x) for x in np.bincount(gid, minlength=len(lens))]
        self.lens = list(lens)                     # by the groups' final numbers
        self.gid = [int(x) for x in gid]
        self.pos = [int(x) for x in np.argsort(gid, kind="stable")]

    def lay(self, groups, mn):
        rows = [None] * len(self.gid)
        i = 0
        for g in groups:
            for x in g:
                rows[self.pos[i]] = x
                i += 1
        assert i == len(rows)
        return rows, [mn + g for g in self.gid]


def _outliers(r, rows, ids, layout, tn, e, ng, mn):
    """e) huge values in rows whose id is nil, and beyond / below an extents
    BAT: they must neither be added nor cause an overflow"""
    huge = _imax(tn)
    extra = [(huge, None), (-huge, None), (huge, None)]
    below = []
    if e is not None:
        extra = [(huge, mn + ng + 2), (huge, mn + ng)] + extra
        below = [(huge, mn - 1), (-huge, mn - 2)]
    if layout == "u":
        for v, g in extra + below:
            i = int(r.integers(0, len(rows) + 1))
            rows.insert(i, v)
            ids.insert(i, g)
        return rows, ids
    return ([v for v, _ in below] + rows + [v for v, _ in extra],
            [g for _, g in below] + ids + [g for _, g in extra])


def _group_cases(tn, tp, cfg, seed=1720):
    """the BATgroupsum calls of one type pair and configuration: the same
    groups in every call but for the planted one (ng // 2), whose rows the
    call's name describes"""
    ng, layout, n = CONFIGS[cfg]
    r = rng(seed + ng + n)
    S, M = _imax(tn), _imax(tp)
    q = _shape(tn, tp)[1]
    img8 = cfg.endswith("img8")
    where = Layout(r, _sizes(r, n, ng), layout)
    sizes = where.lens
    gp = ng // 2
    Lp = sizes[gp]
    base = []
    for j, L in enumerate(sizes):
        if layout == "r":
            base.append([None] if j % 11 == 3 else [int(r.integers(-1 << 40, 1 << 40)) * min(S, M) >> 40])
            continue
        nils = (j % 13 == 5) + (j % 17 == 7) if j != gp and L > 2 else 0
        rows = _seq(r, tn, tp, L - nils, sign=1 if j % 2 else -1)
        if nils and j % 13 == 5:
            rows.insert(0, None)                   # forgotten with several groups
        if nils and j % 17 == 7:
            rows.append(None)                      # the group is nil without skip_nils
        base.append(rows)
    k = 0

    def build(name, planted, skip=True, gate=None):
        nonlocal k
        k += 1
        e = (3, ng) if k % 3 == 0 and not img8 else None
        mn = 3 if e else 0
        sform = None if img8 else SFORMS[k % 4]
        if gate is not None:
            rows, ids = Layout(r, [len(gate)] * ng, layout).lay([gate] * ng, mn)
        else:
            if planted is not None:
                planted = planted + [0] * (Lp - len(planted))
            rows, ids = where.lay(base if planted is None else base[:gp] + [planted] + base[gp + 1:], mn)
        # one row per group: k_gsum_rows wants nothing but the groups' rows
        if not img8 and not (layout == "r" and k % 2):
            rows, ids = _outliers(r, rows, ids, layout, tn, e, ng, mn)
        return GroupCase(name, tn, rows, ids, layout != "u", skip, e, sform, (0, 7)[k // 4 % 2], img8)

    for j in range(2):
        yield build("base %d" % j, None)
        yield build("base %d, nils count" % j, None, False)
    if layout == "r":
        # a value beyond a narrower result type
        if S > M:
            yield build("max", [M])
            yield build("-max", [-M], False)
            yield build("max + 1", [M + 1])
            yield build("-max - 1", [-M - 1], False)
            yield build("-max - 1 again", [-M - 1])
        return
    for open_ in (False, True):
        rows = _gate(tn, tp, 7 if M < 1 << 15 else 50, open_)
        if rows is not None and ng * len(rows) <= 40000:
            yield build("gate open %d" % open_, None, open_, rows)
    if not _feasible(tn, tp, Lp - 3) or Lp < 8:
        if S >= M and Lp > 1:
            # two rows suffice where one value can reach the maximum
            v = M - 3
            yield build("pair exact", [v, 3])
            yield build("pair over", [v, 4])
            yield build("pair -over", [-v, -4], False)
            if Lp > 2:
                yield build("transient", [v, 4, -9])
                yield build("nil, over", [v, None, 4], False)
        return
    ch = (Lp + 255) // 256                         # k_gsum_ordered's rows per lane
    pos = []
    for p in (q, max(ch * 3 - 1, q + 1), Lp - 4):
        if q <= p <= Lp - 3 and p not in pos:
            pos.append(p)
    for j, p in enumerate(pos):
        for sign in (1, -1):
            yield build("exact %d @%d" % (sign, p), _seq(r, tn, tp, Lp - 2, "exact", p, sign), sign > 0)
            yield build("over %d @%d" % (sign, p), _seq(r, tn, tp, Lp - 2, "over", p, sign), sign < 0)
        sign = 1 if j % 2 else -1
        # d) the nil after the planted pair: the error; in front of it: nil
        yield build("over, nil @%d" % p, _seq(r, tn, tp, Lp - 3, "over", p, sign, p + 2), False)
        yield build("nil, over @%d" % p, _seq(r, tn, tp, Lp - 3, "over", p, sign, p), False)
        # a nil before the group's first value: forgotten with several groups
        # (the error), final with one group (nil)
        if ng > 1 or j == 0:
            yield build("nil first, over @%d" % p, _seq(r, tn, tp, Lp - 3, "over", p, sign, 0), False)
        yield build("nils skipped, exact @%d" % p, _seq(r, tn, tp, Lp - 3, "exact", p, -sign, p + 1), True)
    if tn == "hge" and tp == "hge":
        rows = [int(x) for x in r.integers(-9, 10, Lp)]
        for i in (0, Lp // 3, Lp // 2, Lp - 1):
            rows[i] = 1 << 126
        yield build("4 x 2^126", rows)
        rows = [int(x) for x in r.integers(-9, 10, Lp)]
        rows[0] = -(1 << 126) - (1 << 125)
        rows[Lp // 2], rows[Lp // 2 + 1] = 1 << 126, 1 << 126
        yield build("chunk sum 2^127, in range", rows)


def _group_feasible(tn, tp, cfg):
    ng, layout, n = CONFIGS[cfg]
    if layout == "r":
        return _imax(tn) > _imax(tp)
    return _imax(tn) >= _imax(tp) or _feasible(tn, tp, n // ng - n // ng // 4 - 3)


@pytest.mark.parametrize("tn,tp,cfg", GROUP_PARAMS)
def test_oracle_groupsum(ora, tn, tp, cfg):
    """ora_groupsum against the model, and the sweep's ratios"""
    if cfg.endswith("img8"):
        return                                     # the same calls as k2 / k8 for the oracle
    _run_cases(ora, ora, _group_cases(tn, tp, cfg), tp, _group_feasible(tn, tp, cfg), (tn, tp, cfg))


@pytest.mark.gpu
@pytest.mark.parametrize("direct", ["1", "0"])
@pytest.mark.parametrize("tn,tp,cfg", GROUP_PARAMS)
def test_gpu_groupsum(gdk, ora, monkeypatch, tn, tp, cfg, direct):
    """k1 .. k8: the register paths k_gaggr_k<4> / <8> (img8: with BATgroup's
    1-byte ids) and k_gsum_out.  s9 / s300: sorted ids -- gsum_sorted_direct
    (k_gaggr_sorted with SOut, k_gedge_sum) when nils are skipped or absent,
    else, and with MGDK_GSUM_DIRECT=0, k_gaggr_sorted into accumulators and
    k_gsum_out; s9's groups span several 64 x U row ranges, s300's lie within
    one or across one border.  rows: k_gsum_rows.  u300 / u20000: k_gaggr<0>
    (atomics), the planted group's rows far apart.  Behind the gate, always:
    group_rows and k_gsum_ordered."""
    if direct == "0" and CONFIGS[cfg][1] == "u":
        return                                     # MGDK_GSUM_DIRECT only matters for sorted ids
    monkeypatch.setenv("MGDK_GSUM_DIRECT", direct)
    _run_cases(gdk, ora, _group_cases(tn, tp, cfg), tp, _group_feasible(tn, tp, cfg), (tn, tp, cfg))


# ---- the issue's three examples, and the refused types ----------------------


def _examples():
    m62 = 1 << 62
    yield GroupCase("transient", "lng", [m62, 5, m62, 1, -m62, 2], [0, 1, 0, 1, 0, 1], False), "lng"
    yield GroupCase("after a nil", "lng", [1, 5, None, m62, m62, m62], [0, 1, 0, 0, 0, 0], False, False), "lng"
    yield GroupCase("after a nil, one group", "lng", [1, None, m62, m62, m62], [0] * 5, True, False), "lng"
    yield GroupCase("wraps", "hge", [1 << 126] * 4, [0] * 4, True), "hge"


def test_oracle_examples(ora):
    t = _tally()
    for c, tp in _examples():
        _check(ora, ora, c, tp, c.model(tp), t)
    assert t["overflow"] == 2


@pytest.mark.gpu
def test_gpu_examples(gdk, ora):
    t = _tally()
    for c, tp in _examples():
        _check(gdk, ora, c, tp, c.model(tp), t)


def _refused(mod):
    """(call, source name, result name)"""
    oid = _oids(mod, [1, 2, 3])
    b = _bat(mod, "int", [1, 2, 3])
    g = _dense(mod, 0, 3, 0)
    yield (lambda: mod.BATsum(mod.TYPE_lng, oid)), "oid", "lng"
    yield (lambda: mod.BATsum(mod.TYPE_oid, b)), "int", "oid"
    yield (lambda: mod.BATgroupsum(oid, g, None, mod.TYPE_lng)), "oid", "lng"
    yield (lambda: mod.BATgroupsum(b, g, None, mod.TYPE_oid)), "int", "oid"
    yield (lambda: mod.BATgroupsum(b, g, None, mod.TYPE_dbl)), "int", "dbl"


def _check_refused(mod):
    for call, a, b in _refused(mod):
        with pytest.raises(_err(mod)) as e:
            call()
        assert str(e.value) == "type combination (sum(%s)->%s) not supported.\n" % (a, b)


def test_oracle_refused_types(ora):
    _check_refused(ora)


@pytest.mark.gpu
def test_gpu_refused_types(gdk):
    _check_refused(gdk)
