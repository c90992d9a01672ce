"""BATprod / BATgroupprod (gdk_aggr.c:1575-1648 over doprod :1340-1548) with
inputs that multiply.

The arbiter is the rule as oracle/gdk_oracle_grp.c:1502-1510 and
prodminmax.hip:645-707 restate it, through the Python model `_prod_model`
(test_minmax_prod.py) written from that text: integers exact in Python ints,
floats step by step in numpy float32 / float64 in candidate order (one
rounding per step, integers converted with one rounding), so device and
oracle are compared with it bit for bit.  A NaN result (0 * inf) is compared
as "is nil": its sign differs between processors.  The grouped wrapper
`_group_model` restates BATgroupaggrinit: ids outside [min, max] and nil ids
are skipped, empty groups are nil, the result's head is min, an overflow in
any group fails the call; with singleton groups (g dense or key + nonil, e
absent or aligned) the result is BATconvert(b, s, tp): each row's value in the
result type, a nil row nil.

Inputs (`_int_groups` / `_flt_groups`): integer groups multiply factors from
{+-2, +-3} up to the result type's maximum, padded with +-1, so nearly every
product is a large non-zero number (asserted: test_inputs_multiply); explicit
groups sit exactly on the maximum; float groups hold full mantissas in
[0.5, 2) so the rounding order shows, walk through the subnormals and sit on
both sides of the overflow test |v| > 1 && max / |v| < |p|."""
import functools
from fractions import Fraction

import numpy as np
import pytest

from helpers import rng
from test_minmax_prod import _prod_model, _to_float

BITS = {"bte": 8, "sht": 16, "int": 32, "lng": 64, "hge": 128}
IT = {"bte": np.int8, "sht": np.int16, "int": np.int32, "lng": np.int64}
FT = {"flt": np.float32, "dbl": np.float64}
UT = {"flt": np.uint32, "dbl": np.uint64}
EMAX = {"flt": 128, "dbl": 1024}
M64 = (1 << 64) - 1
OID_NIL = 1 << 63
OVERFLOW = "overflow"
# a bound for integer factors multiplied into a float result: far below
# FLT_MAX, far above 2^24, so most steps round
FLOAT_CAP = 1 << 120


def _imax(t):
    return (1 << (BITS[t] - 1)) - 1


def _inil(t):
    return -(1 << (BITS[t] - 1))


# factors whose product is exactly the result type's maximum
EXACT_MAX = {"bte": [127], "sht": [7, 31, 151], "int": [2**31 - 1],
             "lng": [7, 7, 73, 127, 337, 92737, 649657], "hge": [2**127 - 1]}


def test_exact_max_factors():
    for t, fs in EXACT_MAX.items():
        p = 1
        for f in fs:
            p *= f
        assert p == _imax(t), t


# ---- the model --------------------------------------------------------------


def _operand(tn, tp):
    """a non-nil input value as the model's operand"""
    if tp in FT:
        ft = FT[tp]
        return (lambda x: ft(x)) if tn in FT else (lambda x: _to_float(int(x), ft))
    return int


def _fold(rows, tn, tp, skip, ne=True):
    conv = _operand(tn, tp)
    return _prod_model([0 if x is None else conv(x) for x in rows], [x is None for x in rows], tp, skip, ne)


def _group_model(vals, gids, mn, ngrp, tn, tp, skip):
    """BATgroupprod of the candidate rows vals (None: nil) with group ids gids
    (None: nil) over the groups [mn, mn + ngrp): one result per group (None:
    nil), or OVERFLOW"""
    rows = [[] for _ in range(ngrp)]
    for v, g in zip(vals, gids):
        if g is None or g < mn or g >= mn + ngrp:
            continue
        rows[g - mn].append(v)
    out = []
    for rs in rows:
        w = _fold(rs, tn, tp, skip) if rs else None
        if isinstance(w, str):
            return OVERFLOW
        out.append(w)
    return out


def _convert_model(vals, tn, tp):
    """BATconvert of integer values: nil stays nil, a value outside the result
    type raises"""
    out = []
    for v in vals:
        if v is None:
            out.append(None)
        elif tp in FT:
            out.append(_to_float(int(v), FT[tp]))
        elif abs(int(v)) > _imax(tp):
            return OVERFLOW
        else:
            out.append(int(v))
    return out


def _ovf(w):
    return isinstance(w, str)


def _is_nil(w):
    return w is None or w != w


def test_model_int_to_float_is_one_rounding():
    """the model's conversion against exact round-to-nearest-even, on values
    beyond 2^64 and on the ties where a detour through double rounds twice"""
    r = rng(1601)
    cases = [((1 << 24) + 1) << 70, (((1 << 24) + 1) << 70) + 1, ((1 << 24) + 3) << 70, (1 << 64) + 1,
             (1 << 100) - 1, 2**127 - 1, -(2**127 - 1), ((1 << 53) + 1) << 40, (((1 << 53) + 1) << 40) + 1,
             ((1 << 53) + 3) << 40]
    cases += [int(r.integers(1, 1 << 62)) << int(r.integers(3, 64)) | int(r.integers(0, 1 << 30)) for _ in range(200)]
    for ft, m in ((np.float32, 24), (np.float64, 53)):
        for v in cases:
            x = _to_float(v, ft)
            lo, hi = np.nextafter(x, ft(-np.inf)), np.nextafter(x, ft(np.inf))
            ex = abs(Fraction(float(x)) - v)
            for y in (lo, hi):
                if np.isfinite(y):
                    ey = abs(Fraction(float(y)) - v)
                    assert ex <= ey, (v, x, y)
                    if ex == ey:     # a tie: the even mantissa wins
                        mant = Fraction(float(x)) / Fraction(2) ** (abs(v).bit_length() - m)
                        assert mant.denominator == 1 and mant.numerator % 2 == 0, (v, x)
    # the detour through double differs on the sticky tie
    v = (((1 << 24) + 1) << 70) + 1
    assert _to_float(v, np.float32) != np.float32(float(v))


# ---- inputs -----------------------------------------------------------------


def _fits(v, tn):
    return abs(v) <= _imax(tn)


def _pad(r, fs, n):
    fs = list(fs) + [1 if r.random() < 0.5 else -1 for _ in range(n - len(fs))]
    return [fs[i] for i in r.permutation(len(fs))]


def _signed(rows, sign):
    """the rows with the product's sign made `sign`"""
    neg = sum(x < 0 for x in rows) & 1
    return rows if neg == (sign < 0) else [-rows[0]] + rows[1:]


def _smooth(r, cap, first=1, stop=None):
    """factors from {+-2, +-3} after `first`, drawn until the next would pass
    cap (or until `stop` of them)"""
    fs, mag = [], abs(first)
    while stop is None or len(fs) < stop:
        f = int(r.choice((2, 3)))
        if mag * f > cap:
            break
        mag *= f
        fs.append(f if r.random() < 0.5 else -f)
    return fs


def _put_nils(r, rows, k):
    """nil rows into a group: before its first value, after it, or both"""
    rows = list(rows)
    where = k % 3
    if where != 1:
        rows.insert(0, None)
    if where != 0:
        rows.insert(int(r.integers(1, len(rows) + 1)), None)
    return rows


BIG = {
    ("lng", "flt"): [(1 << 62) + 12345, -((1 << 40) + 1), ((1 << 24) + 1) << 30, (((1 << 24) + 1) << 30) + 1],
    ("lng", "lng"): [(1 << 40) + 12345, -((1 << 50) + 3)],
    ("lng", "hge"): [(1 << 62) + 12345, -((1 << 63) - 1)],
    ("hge", "hge"): [(1 << 90) + 12345, -((1 << 100) - 1), (1 << 64) + 1],
    ("hge", "flt"): [((1 << 24) + 1) << 70, (((1 << 24) + 1) << 70) + 1, ((1 << 24) + 3) << 70,
                     -((1 << 90) + (1 << 40) + 1), (1 << 64) + 1, (1 << 100) - 1, 12345],
    ("hge", "dbl"): [((1 << 53) + 1) << 40, (((1 << 53) + 1) << 40) + 1, ((1 << 53) + 3) << 40, (1 << 64) + 1,
                     -((1 << 100) - 1)],
}


def _int_groups(tn, tp, ng=300, seed=1610):
    """the groups' rows in candidate order (None: nil; an empty list: a group
    without rows)"""
    r = rng(seed)
    cap = FLOAT_CAP if tp in FT else _imax(tp)
    big = BIG.get((tn, tp), [])
    groups = []
    for k in range(ng):
        if k % 37 == 5:
            groups.append([])                                   # empty
            continue
        if k % 41 == 7:
            groups.append([None] * int(r.integers(1, 6)))       # all nil
            continue
        first = big[(k // 5) % len(big)] if big and k % 5 == 1 else 1
        fs = _smooth(r, cap, first, None if r.random() < 0.8 else int(r.integers(1, 12)))
        if first != 1:
            fs.append(first)
        rows = _pad(r, fs, max(len(fs), int(r.integers(1, 121))))
        if k % 11 == 3:
            rows = _put_nils(r, rows, k)
        groups.append(rows)
    # exactly the maximum, both signs, and a power of two below it
    if tp in EXACT_MAX and all(_fits(f, tn) for f in EXACT_MAX[tp]):
        fs = EXACT_MAX[tp]
        groups.append(_signed(_pad(r, fs, len(fs) + 9), 1))
        groups.append(_signed(_pad(r, fs, len(fs) + 4), -1))
    if tp not in FT:
        groups.append(_pad(r, _pow2(BITS[tp] - 2, BITS[tn] - 2), 40))
    return groups


def _pow2(e, emax):
    """2^e as factors 2^j, j <= emax"""
    fs = []
    while e > 0:
        j = min(e, emax)
        fs.append(1 << j)
        e -= j
    return fs


def _fpow2(ft, e, emax=120):
    out = []
    while e != 0:
        j = max(-emax, min(e, emax))
        out.append(ft(2.0 ** j))
        e -= j
    return out


def _flt_groups(tn, tp, ng=300, seed=1620):
    r = rng(seed)
    fi, fr = FT[tn], FT[tp]
    E = EMAX[tp]
    groups = []
    for k in range(ng):
        if k % 37 == 5:
            groups.append([])
            continue
        if k % 41 == 7:
            groups.append([None] * int(r.integers(1, 6)))
            continue
        rows = _balanced(r, fi, fr, int(r.integers(1, 121)))
        if k % 13 == 4:
            rows.insert(int(r.integers(0, len(rows) + 1)), fi(-0.0) if k % 2 else fi(0.0))
        if k % 11 == 3:
            rows = _put_nils(r, rows, k)
        groups.append(rows)
    # below the smallest normal and back up: a flushed subnormal would show
    first = fi(1.2345678)
    groups.append([first] + _fpow2(fi, -(E - 2) - 14) + _fpow2(fi, E + 30))
    # the overflow test's passing side
    groups.append(_fpow2(fi, E - 2) + [fi(2.0)])
    groups.append(_fpow2(fi, E - 1) + [fi(1.5)])
    groups.append(_fpow2(fi, E - 1) + [fi(-1.0)] + [fi(1.9999)])
    if tn == tp:
        mx = np.finfo(fi).max
        groups.append([mx, fi(1.0)])
        groups.append([-mx, fi(0.75), np.nextafter(fi(1.0), fi(0.0))])
    # inf after a zero: 0 * inf, a nil result and no error
    groups.append([fi(3.0), fi(0.0), fi(np.inf), fi(2.0)])
    return groups


def _balanced(r, fi, fr, n):
    """n full-mantissa values in [0.5, 2) with random signs whose running
    product stays near 1 and ends above 1 in magnitude"""
    rows, p = [], fr(1.0)
    while len(rows) < n or abs(p) <= 1:
        u = fi(r.random())
        x = fi(1.0) + u if abs(p) <= 1 else fi(0.5) + u * fi(0.5)
        if len(rows) >= n:
            x = fi(1.5) + u * fi(0.5)
        x = x if r.random() < 0.5 else -x
        rows.append(x)
        p = fr(p * fr(x))
    return rows


def _flt_failing(tn, tp):
    """groups on the overflow test's failing side"""
    fi = FT[tn]
    E = EMAX[tp]
    out = {"pow2_x2": _fpow2(fi, E - 1) + [fi(2.0)],
           "inf_after_value": [fi(3.0), fi(np.inf)]}
    if tn == tp:
        out["max_x_next"] = [np.finfo(fi).max, np.nextafter(fi(1.0), fi(2.0))]
    return out


def _large_group(tn, tp, seed=1630):
    """2^17 rows of one group"""
    r = rng(seed)
    n = 1 << 17
    if tn in FT:
        return _balanced(r, FT[tn], FT[tp], n)
    return _pad(r, _smooth(r, _imax(tp)), n)


@functools.lru_cache(maxsize=None)
def _groups(tn, tp, large=False):
    gs = _flt_groups(tn, tp) if tn in FT else _int_groups(tn, tp)
    if large:
        gs = gs[:60]
        gs.insert(20, _large_group(tn, tp))
        gs.insert(41, _large_group(tn, tp, 1631))
    return gs


def _assemble(groups, seed=1640):
    """the rows of all groups shuffled together, each group's rows keeping
    their order: (values, group ids)"""
    r = rng(seed)
    lens = [len(g) for g in groups]
    gid = r.permutation(np.repeat(np.arange(len(groups)), lens))
    pos = np.argsort(gid, kind="stable")
    vals = [None] * len(gid)
    i = 0
    for g in groups:
        for x in g:
            vals[pos[i]] = x
            i += 1
    return vals, [int(x) for x in gid]


def _column(vals, tn):
    if tn in FT:
        return np.array([np.nan if x is None else x for x in vals], FT[tn])
    if tn == "hge":
        w = [(_inil("hge") if x is None else int(x)) & ((1 << 128) - 1) for x in vals]
        return np.array([[x & M64, x >> 64] for x in w], np.uint64).reshape(-1, 2)
    nil = _inil(tn)
    return np.array([nil if x is None else int(x) for x in vals], IT[tn])


# ---- both libraries behind one face -----------------------------------------


def _is_dev(mod):
    return hasattr(mod, "BAT")


def _bat(mod, tn, arr, hseq=0):
    tp = getattr(mod, "TYPE_" + tn)
    if _is_dev(mod):
        return mod.BAT.from_numpy(tp, arr, hseqbase=hseq, sorted_=False, revsorted=False, key=False, nonil=False)
    return mod.Bat.from_array(tp, arr, hseqbase=hseq)


def _oids(mod, a, hseq=0, sorted_=False, key=False, nonil=False):
    a = np.asarray(a, np.uint64)
    if _is_dev(mod):
        return mod.BAT.from_numpy(mod.TYPE_oid, a, hseqbase=hseq, sorted_=sorted_, revsorted=False, key=key,
                                  nonil=nonil)
    return mod.Bat.from_array(mod.TYPE_oid, a, hseqbase=hseq, sorted_=sorted_, key=key, nonil=nonil)


def _dense(mod, tseq, n, hseq=0):
    return (mod.BAT if _is_dev(mod) else mod.Bat).dense(tseq, n, hseqbase=hseq)


def _err(mod):
    return mod.GDKError if _is_dev(mod) else mod.OracleError


def _result(mod, bn):
    s = bn.s
    if _is_dev(mod):
        return {"hseq": s.hseqbase, "count": s.count, "nil": bool(s.tnil), "nonil": bool(s.tnonil),
                "vals": list(bn.values())}
    return {"hseq": s.hseqbase, "count": s.count, "nil": bool(s.nil), "nonil": bool(s.nonil),
            "vals": list(bn.values())}


def _assert_values(got, want, tp, what):
    assert len(got) == len(want), what
    if tp in FT:
        g = np.asarray(got, FT[tp])
        wn = np.array([_is_nil(w) for w in want], bool)
        assert np.array_equal(np.isnan(g), wn), (what, np.flatnonzero(np.isnan(g) != wn)[:8])
        w = np.array([0 if n else x for x, n in zip(want, wn)], FT[tp])
        ok = wn | (g.view(UT[tp]) == w.view(UT[tp]))
        bad = np.flatnonzero(~ok)
        assert bad.size == 0, (what, bad[:8], g[bad[:8]], w[bad[:8]])
    else:
        nil = _inil(tp)
        w = [nil if x is None else x for x in want]
        g = [int(x) for x in got]
        bad = [i for i in range(len(w)) if w[i] != g[i]]
        assert not bad, (what, bad[:8], [g[i] for i in bad[:8]], [w[i] for i in bad[:8]])


class Form:
    """one call's arguments: b's values, the candidates, g over them, e"""

    def __init__(self, name, tn, bvals, bhseq=0, cand=None, sdense=None, gids=None, gsorted=False, gkey=False,
                 gnonil=False, gdense=None, e=None):
        self.name, self.tn, self.bvals, self.bhseq = name, tn, bvals, bhseq
        self.cand = cand            # positions in b of a materialised s
        self.sdense = sdense        # (first position, count, hseqbase of s)
        self.gids, self.gsorted, self.gkey, self.gnonil, self.gdense = gids, gsorted, gkey, gnonil, gdense
        self.e = e                  # (hseqbase, count)

    def positions(self):
        if self.cand is not None:
            return list(self.cand)
        if self.sdense is not None:
            return list(range(self.sdense[0], self.sdense[0] + self.sdense[1]))
        return list(range(len(self.bvals)))

    def rows(self):
        return [self.bvals[p] for p in self.positions()]

    def ids(self):
        if self.gdense is not None:
            return [self.gdense + i for i in range(len(self.positions()))]
        return self.gids

    def range(self):
        """(min, ngrp) of BATgroupaggrinit"""
        if self.e is not None:
            return self.e
        ids = [g for g in self.ids() if g is not None]
        return (min(ids), max(ids) - min(ids) + 1) if ids else (0, 0)

    def model(self, tp, skip):
        mn, ng = self.range()
        return _group_model(self.rows(), self.ids(), mn, ng, self.tn, tp, skip)

    def call(self, mod, tp, skip):
        pos = self.positions()
        b = _bat(mod, self.tn, _column(self.bvals, self.tn), self.bhseq)
        s = None
        if self.cand is not None:
            s = _oids(mod, [self.bhseq + p for p in pos], sorted_=True, key=True, nonil=True)
        elif self.sdense is not None:
            s = _dense(mod, self.bhseq + self.sdense[0], self.sdense[1], self.sdense[2])
        ghseq = self.bhseq + pos[0]
        if self.gdense is not None:
            g = _dense(mod, self.gdense, len(pos), ghseq)
        else:
            g = _oids(mod, [OID_NIL if x is None else x for x in self.gids], ghseq, self.gsorted, self.gkey,
                      self.gnonil)
        e = _dense(mod, 0, self.e[1], self.e[0]) if self.e is not None else None
        return _result(mod, mod.BATgroupprod(b, g, e, getattr(mod, "TYPE_" + tp), skip, s))

    def check(self, mod, tp, skip, want=None):
        """mod's answer against the model's; returns it"""
        want = self.model(tp, skip) if want is None else want
        what = (self.name, self.tn, tp, skip, "device" if _is_dev(mod) else "oracle")
        if _ovf(want):
            with pytest.raises(_err(mod), match="overflow in product"):
                self.call(mod, tp, skip)
            return want
        got = self.call(mod, tp, skip)
        mn, ng = self.range()
        assert (got["hseq"], got["count"]) == (mn, ng), what
        _assert_values(got["vals"], want, tp, what)
        anynil = any(_is_nil(w) for w in want)
        assert (got["nil"], got["nonil"]) == (anynil, not anynil), what
        return want


def _forms(tn, groups, seed=1650):
    """the argument forms of one set of groups"""
    r = rng(seed)
    vals, gid = _assemble(groups)
    n, ng = len(vals), len(groups)
    yield Form("plain", tn, vals, gids=gid)
    # e aligned: exactly the id range
    yield Form("aligned_e", tn, vals, gids=gid, e=(0, ng))
    # g sorted (every group a run of rows), e longer than the id range
    order = np.argsort(np.array(gid), kind="stable")
    yield Form("sorted_g_long_e", tn, [vals[i] for i in order], gids=[gid[i] for i in order], gsorted=True,
               gnonil=True, e=(0, ng + 7))
    # nil ids and ids outside e's window; the rows with a nil id hold a zero
    # or a factor that overflows every result type
    v2, g2 = list(vals), list(gid)
    foreign = _fpow2(FT[tn], 120)[0] if tn in FT else _imax(tn)
    for p in sorted(int(x) for x in r.choice(n, 40, replace=False)):
        v2.insert(p, 0 if p % 2 else foreign)
        g2.insert(p, None)
    yield Form("nil_ids_e_window", tn, v2, gids=g2, e=(3, ng - 10))
    yield Form("nil_ids", tn, v2, gids=g2)
    # s a materialised subset of b's rows; b's head is not 0
    cand = sorted(int(x) for x in r.choice(n, (n * 7) // 10, replace=False))
    yield Form("s_subset", tn, vals, bhseq=1000, cand=cand, gids=[gid[p] for p in cand])
    # s a dense range with a head of its own, e longer
    yield Form("s_dense", tn, vals, bhseq=500, sdense=(37, n - 100, 5), gids=gid[37:n - 63], e=(0, ng + 3))


INT_PAIRS = [("bte", "bte"), ("bte", "sht"), ("sht", "sht"), ("sht", "int"), ("int", "int"), ("int", "lng"),
             ("lng", "lng"), ("lng", "hge"), ("hge", "hge"), ("int", "hge")]
TOFLT_PAIRS = [("int", "flt"), ("lng", "flt"), ("hge", "flt"), ("hge", "dbl")]
FLT_PAIRS = [("flt", "flt"), ("flt", "dbl"), ("dbl", "dbl")]
CPU_PAIRS = [("int", "lng"), ("int", "hge"), ("lng", "hge"), ("hge", "hge"), ("int", "flt"), ("dbl", "dbl")]


# ---- CPU: the inputs, and the oracle against the model ----------------------


@pytest.mark.parametrize("tn,tp", INT_PAIRS + TOFLT_PAIRS + FLT_PAIRS)
def test_inputs_multiply(tn, tp):
    """over both skip_nils settings at least three quarters of the non-empty
    groups have a non-nil product of magnitude above 1"""
    groups = _groups(tn, tp)
    good = total = 0
    for skip in (True, False):
        for rows in groups:
            if not rows:
                continue
            total += 1
            w = _fold(rows, tn, tp, skip)
            assert not _ovf(w)
            good += (not _is_nil(w)) and abs(w) > 1
    assert good * 4 >= total * 3, (good, total)
    # the shapes the description promises are there
    assert any(not g for g in groups) and any(g and all(x is None for x in g) for g in groups)
    assert any(g and g[0] is None and any(x is not None for x in g) for g in groups)
    assert any(g and g[0] is not None and None in g for g in groups)
    if tp in EXACT_MAX and all(_fits(f, tn) for f in EXACT_MAX[tp]):
        ws = {_fold(g, tn, tp, True) for g in groups[-3:]}
        assert {_imax(tp), -_imax(tp)} <= ws


def test_float_boundary_groups():
    """the passing and failing sides of the overflow test, as the description
    lists them, in the model"""
    for t in ("flt", "dbl"):
        ft, E = FT[t], EMAX[t]
        mx = np.finfo(ft).max
        assert _fold(_fpow2(ft, E - 2) + [ft(2)], t, t, True) == ft(2.0) ** (E - 1)
        assert _fold(_fpow2(ft, E - 1) + [ft(1.5)], t, t, True) == ft(1.5) * ft(2.0) ** (E - 1)
        assert _ovf(_fold(_fpow2(ft, E - 1) + [ft(2)], t, t, True))
        assert _ovf(_fold([mx, np.nextafter(ft(1), ft(2))], t, t, True))
        assert _fold([mx, ft(1)], t, t, True) == mx
        assert _fold([mx, np.nextafter(ft(1), ft(0))], t, t, True) < mx
        assert _ovf(_fold([ft(3), ft(np.inf)], t, t, True))
        assert _is_nil(_fold([ft(3), ft(0), ft(np.inf)], t, t, True))
        # the walk through the subnormals keeps its low bits
        sub = _groups(t, t)[-7]
        tiny = min(abs(_fold(sub[:i], t, t, True)) for i in range(1, len(sub)))
        assert 0 < tiny < np.finfo(ft).tiny
        assert _fold(sub, t, t, True) != 0


@pytest.mark.parametrize("tn,tp", CPU_PAIRS)
def test_oracle_groupprod(ora, tn, tp):
    """ora_groupprod against the model over every argument form"""
    for form in _forms(tn, _groups(tn, tp)):
        for skip in (True, False):
            assert form.check(ora, tp, skip) != OVERFLOW


@pytest.mark.parametrize("tn,tp", [("int", "hge"), ("dbl", "dbl")])
def test_oracle_groupprod_large_groups(ora, tn, tp):
    form = next(_forms(tn, _groups(tn, tp, True)))
    for skip in (True, False):
        assert form.check(ora, tp, skip) != OVERFLOW


def _nan_result_form(tn):
    """0 * inf in the only group that could be nil"""
    ft = FT[tn]
    return next(_forms(tn, [[ft(1.5), ft(-3.0)], [ft(3.0), ft(0.0), ft(np.inf), ft(2.0)], [ft(2.5)]]))


@pytest.mark.parametrize("tn", ["flt", "dbl"])
def test_oracle_nan_result_is_a_nil(ora, tn):
    """a NaN product is the nil of flt / dbl: the result may not claim nonil"""
    want = _nan_result_form(tn).check(ora, tn, True)
    assert [_is_nil(w) for w in want] == [False, True, False]


def _overflow_orders(tn, tp):
    """(name, rows of the changed group, skip_nils, the group's expected
    result or OVERFLOW).  `over` multiplies past the result type's maximum."""
    small = 2 if BITS[tn] < BITS[tp] or tn == "bte" else None
    over = [2] * (BITS[tp] - 1) if small else [_imax(tn) // 3, 7]
    inthge = tp == "hge"
    yield "overflow_before_zero", [3] + over + [0], True, OVERFLOW
    yield "zero_before_overflow", [3, 0] + over, True, 0
    yield "overflow_before_nil", [3] + over + [None], False, OVERFLOW
    yield "nil_before_overflow", [3, None] + over, False, None
    yield "nil_skipped_before_overflow", [3, None] + over, True, OVERFLOW
    # a nil before the first value: forgotten by the integer form, kept by hge
    yield "nil_first_then_overflow", [None] + over, False, None if inthge else OVERFLOW
    yield "nil_first_then_value", [None, 5, -3], False, None if inthge else -15


def _changed(tn, tp, rows):
    groups = list(_groups(tn, tp)[:40])
    groups[17] = rows
    return next(_forms(tn, groups))


@pytest.mark.parametrize("tn,tp", [("int", "lng"), ("bte", "bte"), ("int", "hge"), ("hge", "hge")])
def test_oracle_overflow_orders(ora, tn, tp):
    for name, rows, skip, expect in _overflow_orders(tn, tp):
        form = _changed(tn, tp, rows)
        want = form.model(tp, skip)
        assert (want if _ovf(want) else want[17]) == expect, name
        form.check(ora, tp, skip, want)


def _int_boundary(tn, tp):
    """(name, rows, expected product or OVERFLOW) around an integer result
    type's maximum: exactly the maximum in both signs passes, twice it fails
    in both signs, and so does 2^(bits-2) * (+-2) -- the negative one lands on
    -2^(bits-1), the bit pattern of nil, which a test against the type's
    minimum instead of -maximum would let through"""
    mx = _imax(tp)
    if all(_fits(f, tn) for f in EXACT_MAX[tp]):
        fs = EXACT_MAX[tp]
        yield "max", [-1] + fs + [-1], mx
        yield "neg_max", fs + [-1], -mx
        yield "max_x2", fs + [2], OVERFLOW
        yield "max_x_neg2", fs + [-2], OVERFLOW
        yield "neg2_x_max", [-2] + fs, OVERFLOW
    p2 = _pow2(BITS[tp] - 2, BITS[tn] - 2)
    yield "pow2", p2 + [-1], -(1 << (BITS[tp] - 2))
    yield "pow2_x2", p2 + [2], OVERFLOW
    yield "pow2_x_neg2", p2 + [-2], OVERFLOW
    yield "neg2_x_pow2", [-2] + p2, OVERFLOW


def _check_int_boundary(mod, tn, tp):
    """each boundary group inside a grouped call and as a whole column"""
    ttp = getattr(mod, "TYPE_" + tp)
    for name, rows, expect in _int_boundary(tn, tp):
        assert _fold(rows, tn, tp, True) == expect, name
        form = _changed(tn, tp, rows)
        for skip in (True, False):
            want = form.check(mod, tp, skip)
            assert (want if _ovf(want) else want[17]) == expect, name
        b = _bat(mod, tn, _column(rows, tn))
        if _ovf(expect):
            with pytest.raises(_err(mod), match="overflow in product"):
                mod.BATprod(ttp, b, None, True, True)
        else:
            assert int(mod.BATprod(ttp, b, None, True, True)) == expect, name


@pytest.mark.parametrize("tn,tp", INT_PAIRS)
def test_oracle_integer_boundary(ora, tn, tp):
    _check_int_boundary(ora, tn, tp)


def _one_group_forms(tn, tp):
    """one group among rows that are not its own.  The foreign rows hold a
    zero (folding them in gives 0) or a factor that overflows (folding it in
    fails the call)."""
    r = rng(1660)
    if tn in FT:
        rows = _balanced(r, FT[tn], FT[tp], 4000)
        zero, over = FT[tn](0.0), _fpow2(FT[tn], 120)[0]
        over_rows = [over] * (EMAX[tp] // 120 + 1)
    else:
        rows = _pad(r, _smooth(r, FLOAT_CAP if tp in FT else _imax(tp)), 4000)
        zero, over_rows = 0, [_imax(tn)] * ((EMAX[tp] if tp in FT else BITS[tp]) // (BITS[tn] - 1) + 1)
    rows.insert(5, None)
    # no nil id and no e: the range is that of g's own ids, nothing is foreign
    yield Form("one_group_nonil_g", tn, rows, gids=[7] * len(rows), gsorted=True, gnonil=True)
    for foreign, tag in (([zero] * 6, "zero"), (over_rows * 3, "overflow")):
        vals, gid = list(rows), [7] * len(rows)
        for x in foreign:
            p = int(r.integers(0, len(vals) // 2))
            vals.insert(p, x)
            gid.insert(p, None)
        yield Form("one_group_nil_ids_" + tag, tn, vals, gids=gid)
        yield Form("one_group_e1_" + tag, tn, vals, gids=[0 if g == 7 else 1 for g in gid], e=(0, 1))


ONE_GROUP_PAIRS = [("int", "lng"), ("hge", "hge"), ("dbl", "dbl"), ("int", "flt")]


@pytest.mark.parametrize("tn,tp", ONE_GROUP_PAIRS)
def test_oracle_one_group(ora, tn, tp):
    for form in _one_group_forms(tn, tp):
        for skip in (True, False):
            want = form.check(ora, tp, skip)
            assert want != OVERFLOW and len(want) == 1
            assert skip is False or (not _is_nil(want[0]) and abs(want[0]) > 1)


def _singleton_forms(tn):
    r = rng(1670)
    n = 3000
    lim = min(_imax(tn), 2**31 - 1)
    vals = [int(x) for x in r.integers(-lim, lim + 1, n)]
    for p in r.choice(n, 60, replace=False):
        vals[int(p)] = None
    vals[3] = 0
    yield Form("key_nonil_g", tn, vals, gids=list(range(n)), gsorted=True, gkey=True, gnonil=True)
    yield Form("key_nonil_g_aligned_e", tn, vals, gids=list(range(n)), gsorted=True, gkey=True, gnonil=True,
               e=(0, n))
    yield Form("dense_g", tn, vals, gdense=0)
    # ids in another order: still BATconvert(b), the rows' order
    yield Form("key_nonil_g_permuted", tn, vals, gids=[int(x) for x in r.permutation(n)], gkey=True, gnonil=True)


def _check_singletons(mod, form, tp, skip):
    want = _convert_model(form.bvals, form.tn, tp)
    what = (form.name, form.tn, tp, skip)
    if _ovf(want):
        with pytest.raises(_err(mod)) as e:
            form.call(mod, tp, skip)
        return str(e.value)
    got = form.call(mod, tp, skip)
    assert (got["hseq"], got["count"]) == (0, len(want)), what
    _assert_values(got["vals"], want, tp, what)
    assert (got["nil"], got["nonil"]) == (True, False), what
    return None


@pytest.mark.parametrize("tp", ["lng", "hge", "dbl"])
def test_oracle_singleton_groups(ora, tp):
    """the shortcut of gdk_aggr.c:1604-1611: a nil row stays nil with
    skip_nils too (doprod would answer 1 for hge, nil otherwise)"""
    for form in _singleton_forms("int"):
        for skip in (True, False):
            _check_singletons(ora, form, tp, skip)


def _lng_to_int_forms(fits):
    form = next(_singleton_forms("lng"))
    if not fits:
        form.bvals = list(form.bvals)
        form.bvals[1234] = 1 << 40
    return form


def test_oracle_singleton_groups_narrowing(ora):
    """lng to int is no product type pair, but the shortcut comes first"""
    _check_singletons(ora, _lng_to_int_forms(True), "int", True)
    assert _check_singletons(ora, _lng_to_int_forms(False), "int", True)
    # with two rows in a group the type check is reached
    form = next(_singleton_forms("lng"))
    form.gids = [0] + form.gids[:-1]
    form.gkey = False
    with pytest.raises(ora.OracleError, match="not supported"):
        form.call(ora, "int", True)


# ---- the whole column: the model over a compressed column -------------------


def _chunking(n):
    """prod_parts' cut of n rows: (rows per workgroup, workgroups)"""
    chunk = 256 * 64 if n < 256 * 64 else (n + 1023) // 1024
    return chunk, (n + chunk - 1) // chunk


def _boundaries(n):
    """first and last rows of lane runs, in the first, last and middle
    workgroups' chunks"""
    chunk, nb = _chunking(n)
    out = set()
    for c in {0, 1, nb // 3, nb // 2, nb - 2, nb - 1} | set(range(0, nb, max(1, nb // 24))):
        if not 0 <= c < nb:
            continue
        b0, b1 = c * chunk, min(n, (c + 1) * chunk)
        per = (b1 - b0 + 255) // 256
        for t in range(256) if nb <= 2 else sorted(set(range(0, 256, 5)) | {1, 2, 127, 128, 253, 254, 255}):
            r0, r1 = b0 + per * t, min(b1, b0 + per * (t + 1))
            if r0 < r1:
                out.update((r0, r1 - 1))
    return sorted(out)


class Column:
    """+-1 everywhere but at a few rows: `special` (row: value) and the nil
    rows `nil` (a bool array)"""

    def __init__(self, n, seed):
        self.n = n
        self.base = np.where(rng(seed).random(n) < 0.5, 1, -1).astype(np.int64)
        self.nil = np.zeros(n, bool)
        self.special = {}

    def array(self, tn):
        if tn == "hge":
            a = np.stack([self.base.view(np.uint64), (self.base >> 63).view(np.uint64)], axis=1)
            for p, x in self.special.items():
                w = x & ((1 << 128) - 1)
                a[p] = (w & M64, w >> 64)
            a[self.nil] = (0, 1 << 63)
            return a
        a = self.base.astype(IT[tn])
        for p, x in self.special.items():
            assert _fits(x, tn)
            a[p] = x
        a[self.nil] = _inil(tn)
        return a

    def sequence(self, rows=None):
        """the candidate rows as a short equivalent sequence: a run of +-1
        rows is one +-1 (their product: no row of it can overflow, and one
        value marks the group seen as well as many), a run of nils one nil"""
        rows = np.arange(self.n) if rows is None else rows
        code = np.zeros(len(rows), np.int8)
        code[self.nil[rows]] = 1
        sp = np.flatnonzero(np.isin(rows, np.fromiter(self.special, np.int64, len(self.special))))
        sp = sp[~self.nil[rows[sp]]]
        code[sp] = 2
        starts = np.unique(np.concatenate([[0], np.flatnonzero(np.diff(code)) + 1, sp, sp + 1]))
        starts = starts[starts < len(rows)]
        cneg = np.concatenate([[0], np.cumsum(self.base[rows] < 0)])
        seq = []
        for a, b in zip(starts, np.append(starts[1:], len(rows))):
            if code[a] == 0:
                seq.append(-1 if (cneg[b] - cneg[a]) & 1 else 1)
            elif code[a] == 1:
                seq.append(None)
            else:
                seq.append(self.special[int(rows[a])])
        return seq


def _col_factors(r, tn, tp, exact):
    """factors with a product of exactly the maximum (`exact`, where the
    input type holds them), else from {2, 3} up to more than half of it"""
    if exact:
        return list(EXACT_MAX[tp]) if all(_fits(f, tn) for f in EXACT_MAX[tp]) else None
    fs = [abs(f) for f in _smooth(r, _imax(tp))]
    mag = 1
    for f in fs:
        mag *= f
    while mag * 2 <= _imax(tp):
        mag *= 2
        fs.append(2)
    return fs


def _col_cases(n, tn, tp, seed):
    """(name, Column) over the orders of first value, nil, zero and the
    overflowing factors that change the answer"""
    r = rng(seed)
    bnd = _boundaries(n)

    def at(frac):
        return bnd[min(len(bnd) - 1, int(frac * len(bnd)))]

    def spread(col, fs, lo=0):
        ps = [p for p in bnd if p >= lo and p not in col.special and not col.nil[p]]
        assert len(ps) >= len(fs), (n, len(ps), len(fs))
        for p, f in zip(sorted(int(x) for x in r.choice(ps, len(fs), replace=False)), fs):
            col.special[p] = f

    def cluster(col, fs, p):
        """the factors on the rows from p on (they multiply past the maximum)"""
        for i, f in enumerate(fs):
            assert p + i not in col.special
            col.special[p + i] = f

    smooth = _col_factors(r, tn, tp, False)
    over = smooth + [2]
    p1, p2, p3 = at(0.2), at(0.5), at(0.8)
    assert p1 + len(over) < p2 and p2 + len(over) < p3 and p3 + len(over) < n
    for exact in (True, False):
        fs = _col_factors(r, tn, tp, exact)
        if fs is None:
            continue
        tag = "exact_max" if exact else "smooth"
        c = Column(n, seed)
        spread(c, fs)
        yield tag, c
        c = Column(n, seed + 1)
        spread(c, fs + [2])
        yield tag + "_x2", c
    c = Column(n, seed + 2)
    c.nil[:p1] = True
    spread(c, smooth, p1)
    yield "nils_before_first_value", c
    c = Column(n, seed + 3)
    c.nil[:p1] = True
    cluster(c, over, p2)
    c.nil[p3] = True
    yield "nils_first_overflow_nil", c
    c = Column(n, seed + 4)
    c.nil[:p1] = True
    c.nil[p2] = True
    cluster(c, over, p3)
    yield "nils_first_nil_overflow", c
    c = Column(n, seed + 5)
    cluster(c, over, p1)
    c.nil[p2] = True
    c.special[p3] = 0
    yield "overflow_nil_zero", c
    c = Column(n, seed + 6)
    c.nil[p1] = True
    cluster(c, over, p2)
    c.special[p3] = 0
    yield "nil_overflow_zero", c
    c = Column(n, seed + 7)
    c.nil[p1] = True
    c.special[p2] = 0
    cluster(c, over, p3)
    yield "nil_zero_overflow", c
    c = Column(n, seed + 8)
    c.special[p1] = 0
    c.nil[p2] = True
    cluster(c, over, p3)
    yield "zero_nil_overflow", c
    c = Column(n, seed + 9)
    cluster(c, smooth, p1)
    c.special[p2] = 0
    cluster(c, over, p3)
    yield "value_zero_overflow", c
    c = Column(n, seed + 10)
    c.nil[:n - 1] = True
    c.special[n - 1] = 5
    yield "first_value_is_last_row", c
    c = Column(n, seed + 11)
    c.nil[0] = True
    spread(c, smooth, 1)
    yield "nil_at_row_0", c
    # the overflow and the zero in neighbouring lane runs and in neighbouring
    # chunks, in both orders: a combine that takes two of them out of order
    # loses the overflow or finds one that the zero hides
    chunk, nb = _chunking(n)
    starts = []
    for ch in (0, nb // 2):
        b0 = ch * chunk
        per = (min(n, b0 + chunk) - b0 + 255) // 256
        starts += [b0 + 2 * per, b0 + 3 * per] + ([b0] if ch else [])
    # both inside one lane run, where few factors of the input type's maximum
    # pass the result's
    big = [_imax(tn)] * (BITS[tp] // (BITS[tn] - 1) + 1)
    per0 = (min(n, chunk) + 255) // 256
    if len(big) + 1 <= per0:
        c = Column(n, seed + 12)
        c.special[2 * per0] = 0
        cluster(c, big, 2 * per0 + 1)
        yield "zero_then_overflow_in_one_run", c
        c = Column(n, seed + 13)
        cluster(c, big, 2 * per0)
        c.special[2 * per0 + len(big)] = 0
        yield "overflow_then_zero_in_one_run", c
    for i, s in enumerate(x for x in starts if len(over) < x < n - len(over)):
        c = Column(n, seed + 20 + i)
        cluster(c, over, s - len(over))
        c.special[s] = 0
        yield "overflow_then_zero_at_%d" % s, c
        c = Column(n, seed + 30 + i)
        c.special[s - 1] = 0
        cluster(c, over, s)
        yield "zero_then_overflow_at_%d" % s, c


def _col_results(tn, n):
    out = [t for t in ("lng", "hge") if BITS[t] >= BITS[tn]]
    return out + ["bte"] if tn == "bte" and n == 16385 else out


def _check_column(mods, n, tn):
    outcomes = set()
    for tp in _col_results(tn, n):
        for name, col in _col_cases(n, tn, tp, 1700 + BITS[tn]):
            arr = col.array(tn)
            keep = rng(1790).random(n) < 0.6
            keep[col.nil] = True
            keep[np.fromiter(col.special, np.int64, len(col.special))] = True
            cand = np.flatnonzero(keep)
            for rows in (None, cand):
                seq = col.sequence(rows)
                vals, isn = [0 if x is None else x for x in seq], [x is None for x in seq]
                for mod in mods:
                    b = _bat(mod, tn, arr)
                    s = _oids(mod, rows, sorted_=True, key=True, nonil=True) if rows is not None else None
                    for skip in (True, False):
                        for ne in (True, False):
                            want = _prod_model(vals, isn, tp, skip, ne)
                            what = (name, n, tn, tp, rows is not None, skip, ne, _is_dev(mod))
                            outcomes.add(want if _ovf(want) or want is None or want == 0 else "value")
                            if _ovf(want):
                                with pytest.raises(_err(mod), match="overflow in product"):
                                    mod.BATprod(getattr(mod, "TYPE_" + tp), b, s, skip, ne)
                                continue
                            got = mod.BATprod(getattr(mod, "TYPE_" + tp), b, s, skip, ne)
                            assert int(got) == (_inil(tp) if want is None else want), what
                            if name == "exact_max":
                                assert abs(want) == _imax(tp), what
    assert outcomes == {OVERFLOW, None, 0, "value"}


def test_column_sequence_is_the_column():
    """the compressed sequence against the plain loop over every row"""
    n = 3001
    for name, col in _col_cases(n, "int", "lng", 1732):
        arr = col.array("int")
        for rows in (None, np.flatnonzero(rng(1733).random(n) < 0.5)):
            a = arr if rows is None else arr[rows]
            seq = col.sequence(rows)
            for skip in (True, False):
                for ne in (True, False):
                    for tp in ("lng", "hge"):
                        full = _prod_model([int(x) for x in a], list(a == _inil("int")), tp, skip, ne)
                        short = _prod_model([0 if x is None else x for x in seq], [x is None for x in seq], tp,
                                            skip, ne)
                        assert full == short, (name, skip, ne, tp)


@pytest.mark.parametrize("n", [16383, 16384, 16385])
@pytest.mark.parametrize("tn", ["bte", "int", "lng", "hge"])
def test_oracle_prod_column(ora, n, tn):
    _check_column([ora], n, tn)


# ---- device -----------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("tn,tp", INT_PAIRS[:-1] + TOFLT_PAIRS + FLT_PAIRS)
def test_gpu_groupprod_forms(gdk, ora, tn, tp):
    """every group of every argument form: the device against the model, and
    the oracle against the same"""
    for form in _forms(tn, _groups(tn, tp)):
        for skip in (True, False):
            want = form.model(tp, skip)
            assert want != OVERFLOW
            form.check(gdk, tp, skip, want)
            form.check(ora, tp, skip, want)


@pytest.mark.gpu
@pytest.mark.parametrize("tn,tp", [("int", "hge"), ("dbl", "dbl")])
def test_gpu_groupprod_large_groups(gdk, tn, tp):
    """two groups of 2^17 rows among small ones, their rows spread over many
    blocks of the sort by group: the dbl one pins the order within a group"""
    form = next(_forms(tn, _groups(tn, tp, True)))
    for skip in (True, False):
        assert form.check(gdk, tp, skip) != OVERFLOW


@pytest.mark.gpu
@pytest.mark.parametrize("tn,tp", [("int", "lng"), ("bte", "bte"), ("int", "hge"), ("hge", "hge")])
def test_gpu_overflow_orders(gdk, tn, tp):
    for name, rows, skip, expect in _overflow_orders(tn, tp):
        form = _changed(tn, tp, rows)
        want = form.model(tp, skip)
        assert (want if _ovf(want) else want[17]) == expect, name
        form.check(gdk, tp, skip, want)


@pytest.mark.gpu
@pytest.mark.parametrize("tn,tp", INT_PAIRS)
def test_gpu_integer_boundary(gdk, tn, tp):
    """the maximum, twice it and 2^(bits-2) * (+-2) for every integer result
    type, grouped and as a whole column"""
    _check_int_boundary(gdk, tn, tp)


@pytest.mark.gpu
@pytest.mark.parametrize("tn,tp", FLT_PAIRS + [("hge", "flt")])
def test_gpu_float_overflow_boundary(gdk, ora, tn, tp):
    """the failing side of the float overflow test fails the call on both"""
    if tn not in FT:
        rows = {"past_max": [1 << 100, 1 << 100]}
    else:
        rows = _flt_failing(tn, tp)
    for name, rs in rows.items():
        form = _changed(tn, tp, rs)
        for mod in (gdk, ora):
            assert form.check(mod, tp, True) == OVERFLOW, name


@pytest.mark.gpu
@pytest.mark.parametrize("tn", ["flt", "dbl"])
def test_gpu_nan_result_is_a_nil(gdk, tn):
    want = _nan_result_form(tn).check(gdk, tn, True)
    assert [_is_nil(w) for w in want] == [False, True, False]


@pytest.mark.gpu
@pytest.mark.parametrize("tn,tp", ONE_GROUP_PAIRS)
def test_gpu_one_group(gdk, tn, tp):
    """one group: rows with a nil id or an id beyond e are not its rows"""
    for form in _one_group_forms(tn, tp):
        for skip in (True, False):
            assert form.check(gdk, tp, skip) != OVERFLOW


@pytest.mark.gpu
@pytest.mark.parametrize("tp", ["lng", "hge", "dbl"])
def test_gpu_singleton_groups(gdk, tp):
    for form in _singleton_forms("int"):
        for skip in (True, False):
            _check_singletons(gdk, form, tp, skip)


@pytest.mark.gpu
def test_gpu_singleton_groups_narrowing(gdk):
    _check_singletons(gdk, _lng_to_int_forms(True), "int", True)
    form = _lng_to_int_forms(False)
    msg = _check_singletons(gdk, form, "int", True)
    with pytest.raises(gdk.GDKError) as e:
        gdk.BATconvert(_bat(gdk, "lng", _column(form.bvals, "lng")), None, gdk.TYPE_int)
    assert msg == str(e.value)
    form = next(_singleton_forms("lng"))
    form.gids = [0] + form.gids[:-1]
    form.gkey = False
    with pytest.raises(gdk.GDKError, match="not supported"):
        form.call(gdk, "int", True)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16383, 16384, 16385, 1_000_003])
@pytest.mark.parametrize("tn", ["bte", "int", "lng", "hge"])
def test_gpu_prod_column(gdk, ora, n, tn):
    """the parallel integer BATprod: factors on the first and last rows of
    lane runs and chunks, products of exactly the maximum and twice it, and
    first value / nil / zero / overflow each in another chunk, in every order
    that changes the answer; with and without candidates"""
    _check_column([gdk, ora], n, tn)
