"""The ranking window functions SQLrow_number, SQLrank, SQLdense_rank,
SQLpercent_rank and SQLcume_dist (sql/backends/monet5/sql_rank.c) over the
partition bits p and peer bits o.

The reference here is the plain loops of `loops` below (the contract of
DESIGN.md 11.7); `model` is their vectorised form (prefix maximum, cumulative
sum and suffix minimum over the flags), checked against the loops on the CPU
and used for the large columns.  Every device result is compared bit for bit.
"""
import itertools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("row_number", "rank", "dense_rank", "percent_rank", "cume_dist")
FORMS = ((True, True), (True, False), (False, True), (False, False))     # (p given, o given)
BIG = (1 << 20) + 3


# ---- the reference --------------------------------------------------------------

def loops(fn, n, p, o):
    """sql_rank.c's loops, row by row.  p / o: int8 arrays or None."""
    def P(i):
        return i == 0 or (p is not None and p[i] != 0)

    def O(i):
        return o is not None and o[i] != 0

    if fn in ("row_number", "rank", "dense_rank"):
        r = np.zeros(n, np.int32)
        j = k = 1
        for i in range(n):
            if fn == "row_number":
                if P(i):
                    j = 1
                r[i] = j
                j += 1
            elif fn == "rank":
                if P(i):
                    j = k = 1
                elif O(i):
                    j = k
                r[i] = j
                k += 1
            else:
                if P(i):
                    j = 1
                elif O(i):
                    j += 1
                r[i] = j
        return r
    r = np.zeros(n, np.float64)
    a = 0
    while a < n:
        e = a + 1
        while e < n and not P(e):
            e += 1
        cnt = e - a
        x = a
        while x < e:
            y = x + 1
            while y < e and not O(y):
                y += 1
            for i in range(x, y):
                if fn == "percent_rank":
                    r[i] = 0.0 if cnt == 1 else np.float64(x - a) / np.float64(cnt - 1)
                else:
                    r[i] = np.float64(y - a) / np.float64(cnt)
            x = y
        a = e
    return r


def parts(n, p, o):
    """per row: partition start a, peer start x, partition end e, peer end y,
    and d = the peer bits since a"""
    idx = np.arange(n, dtype=np.int64)
    P = np.zeros(n, bool) if p is None else np.asarray(p[:n]) != 0
    O = np.zeros(n, bool) if o is None else np.asarray(o[:n]) != 0
    if n:
        P[0] = True
    S = P | O
    a = np.maximum.accumulate(np.where(P, idx, 0))
    x = np.maximum.accumulate(np.where(S, idx, 0))
    e = np.append(np.minimum.accumulate(np.where(P, idx, n)[::-1])[::-1][1:], n)[:n]
    y = np.append(np.minimum.accumulate(np.where(S, idx, n)[::-1])[::-1][1:], n)[:n]
    c = np.cumsum(O & ~P)
    d = c - c[a] if n else c
    return a, x, e, y, d


def model(fn, n, p, o):
    a, x, e, y, d = parts(n, p, o)
    if fn == "row_number":
        return (np.arange(n, dtype=np.int64) - a + 1).astype(np.int32)
    if fn == "rank":
        return (x - a + 1).astype(np.int32)
    if fn == "dense_rank":
        return (d + 1).astype(np.int32)
    cnt = e - a
    if fn == "percent_rank":
        den = np.where(cnt == 1, 1, cnt - 1).astype(np.float64)
        return np.where(cnt == 1, 0.0, (x - a).astype(np.float64) / den)
    return (y - a).astype(np.float64) / cnt.astype(np.float64)


def rng(seed):
    return np.random.default_rng(seed)


# ---- CPU ------------------------------------------------------------------------

def test_model_equals_loops():
    r = rng(11)
    for _ in range(300):
        n = int(r.integers(1, 61))
        dens = r.random(2)
        p = r.choice(np.array([0, 1, -128], np.int8), n, p=[1 - dens[0], dens[0] / 2, dens[0] / 2])
        o = r.choice(np.array([0, 1, -128], np.int8), n, p=[1 - dens[1], dens[1] / 2, dens[1] / 2])
        for hp, ho in FORMS:
            pp, oo = p if hp else None, o if ho else None
            for fn in FUNCS:
                want, got = loops(fn, n, pp, oo), model(fn, n, pp, oo)
                assert want.dtype == got.dtype
                assert np.array_equal(want.view(np.uint8), got.view(np.uint8)), (fn, hp, ho, p, o)


def test_header_declares_rank_functions():
    txt = open(os.path.join(ROOT, "include", "mgdk.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for f in ("mgdk_SQLrow_number", "mgdk_SQLrank", "mgdk_SQLdense_rank", "mgdk_SQLpercent_rank",
              "mgdk_SQLcume_dist"):
        assert re.search(r"mgdk_bat\s*\*\s*%s\s*\(" % f, txt), f


# ---- GPU ------------------------------------------------------------------------

def call(gdk, fn, b, p, o):
    if fn == "row_number":
        return gdk.SQLrow_number(b, p)
    return getattr(gdk, "SQL" + fn)(b, p, o)


def bits(gdk, f):
    return gdk.BAT.from_numpy(gdk.TYPE_bit, np.asarray(f, np.int8))


def rows(gdk, n, hseq=0):
    """a column that supplies count and hseqbase only"""
    return gdk.BAT.from_numpy(gdk.TYPE_int, np.zeros(n, np.int32), hseqbase=hseq)


def same(gdk, got, want, n, hseq, what):
    s = got.s
    assert s.ttype == (gdk.TYPE_int if want.dtype == np.int32 else gdk.TYPE_dbl), what
    assert s.count == n and s.hseqbase == hseq, what
    assert s.tnonil == 1 and s.tnil == 0, what
    assert bool(s.tsorted) == bool(s.trevsorted) == bool(s.tkey) == (n <= 1), what
    g = got.to_numpy()
    assert g.dtype == want.dtype, what
    assert np.array_equal(g.view(np.uint8), want.view(np.uint8)), \
        (what, np.flatnonzero(g.view(np.uint64 if g.itemsize == 8 else np.uint32) !=
                              want.view(np.uint64 if g.itemsize == 8 else np.uint32))[:8])


def check(gdk, n, p, o, b=None, hseq=0, forms=FORMS, funcs=FUNCS, P=None, O=None):
    """all of funcs in all of forms over the bits p, o against the model"""
    b = rows(gdk, n, hseq) if b is None else b
    P = bits(gdk, p) if P is None else P
    O = bits(gdk, o) if O is None else O
    for hp, ho in forms:
        for fn in funcs:
            want = model(fn, n, p if hp else None, o if ho else None)
            got = call(gdk, fn, b, P if hp else None, O if ho else None)
            same(gdk, got, want, n, hseq, (fn, hp, ho))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_exhaustive_small(gdk, n):
    pats = [np.array(t, np.int8) for t in itertools.product((0, 1), repeat=n)]
    bats = [bits(gdk, t) for t in pats]
    b = rows(gdk, n)
    want = {}
    for fn in FUNCS:
        for ip, p in enumerate(pats):
            want[fn, ip, None] = loops(fn, n, p, None)
            want[fn, None, ip] = loops(fn, n, None, p)
            for io, o in enumerate(pats):
                want[fn, ip, io] = loops(fn, n, p, o)
        want[fn, None, None] = loops(fn, n, None, None)
    for (fn, ip, io), w in want.items():
        got = call(gdk, fn, b, None if ip is None else bats[ip], None if io is None else bats[io])
        same(gdk, got, w, n, 0, (fn, ip, io))


@pytest.mark.gpu
def test_empty(gdk):
    z = np.zeros(0, np.int8)
    check(gdk, 0, z, z)
    check(gdk, 0, z, z, b=gdk.BAT.dense(0, 0, hseqbase=3), hseq=3)


def layout(r, n, kind):
    """tests/test_gpu_window_funcs.py::_layout"""
    if kind == "one":
        p = np.zeros(n, np.int8)
    elif kind == "small":
        p = (r.random(n) < 0.2).astype(np.int8)
    else:
        p = (r.random(n) < 0.002).astype(np.int8)
    p[0] = 0
    o = np.maximum(p, (r.random(n) < 0.4).astype(np.int8))
    o[0] = 0
    return p, o


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["one", "small", "large"])
@pytest.mark.parametrize("variant", ["plain", "free_o", "nil_bits", "row0_set", "int_hseq7", "void"])
def test_random(gdk, kind, variant):
    n = 100_003
    r = rng(len(kind) * 7 + len(variant))
    p, o = layout(r, n, kind)
    b, hseq = None, 0
    if variant == "free_o":
        # peer bits that do not follow the partition bits: a partition start
        # still starts a peer group
        o = (r.random(n) < 0.3).astype(np.int8)
    elif variant == "nil_bits":
        p = np.where((p != 0) & (r.random(n) < 0.5), -128, p).astype(np.int8)
        o = np.where((o != 0) & (r.random(n) < 0.5), -128, o).astype(np.int8)
        o[5] = -128
    elif variant == "row0_set":
        p[0] = 1
        o[0] = 1
    elif variant == "int_hseq7":
        b, hseq = gdk.BAT.from_numpy(gdk.TYPE_int, r.integers(-5, 5, n).astype(np.int32), hseqbase=7), 7
    elif variant == "void":
        b, hseq = gdk.BAT.dense(40, n, hseqbase=2), 2
    check(gdk, n, p, o, b=b, hseq=hseq)


def edge_layout():
    """starts on the first and last row of a tile for every tile length 2^8 ..
    2^14 (and one row into it), tiles without any start, peer starts one row
    after every partition start and at random elsewhere"""
    n = BIG
    r = rng(77)
    p = np.zeros(n, np.int8)
    for m in range(8, 15):
        ks = np.unique(np.concatenate([[1, 2, (n >> m) - 1, n >> m], r.integers(1, n >> m, 6)]))
        for k in ks:
            for at in (k << m, (k << m) - 1, (k << m) + 1):
                if 0 < at < n:
                    p[at] = 1
    o = (r.random(n) < 1e-4).astype(np.int8)
    at = np.flatnonzero(p) + 1
    o[at[at < n]] = 1
    # 40000 rows (more than two tiles of the largest length) with no start
    p[300_000:340_000] = 0
    o[300_000:340_000] = 0
    return p, o


@pytest.mark.gpu
def test_tile_edges(gdk):
    p, o = edge_layout()
    check(gdk, BIG, p, o)


def carry_layout(kind):
    n = BIG
    p, o = np.zeros(n, np.int8), np.zeros(n, np.int8)
    if kind == "no_start":            # every tile's answer is the carry
        pass
    elif kind == "peer_at_end":
        o[n - 1] = 1
    elif kind == "p_at_n_minus_2":
        p[n - 2] = 1
    elif kind == "all_p":
        p[:] = 1
    else:                             # all_o: every row a peer start in one partition
        o[:] = 1
    return p, o


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["no_start", "peer_at_end", "p_at_n_minus_2", "all_p", "all_o"])
def test_long_carries(gdk, kind):
    p, o = carry_layout(kind)
    check(gdk, BIG, p, o)


@pytest.mark.gpu
def test_values(gdk):
    n = 200_001
    r = rng(5)
    p = (r.random(n) < 0.3).astype(np.int8)          # many one-row partitions
    p[100_000:150_000] = 0
    o = (r.random(n) < 0.3).astype(np.int8)
    a, x, e, y, _ = parts(n, p, o)
    b, P, O = rows(gdk, n), bits(gdk, p), bits(gdk, o)
    pr = gdk.SQLpercent_rank(b, P, O).to_numpy()
    cd = gdk.SQLcume_dist(b, P, O).to_numpy()
    one = e - a == 1
    assert one.sum() > 1000 and (~one).sum() > 1000
    assert not np.isnan(pr).any() and not np.isnan(cd).any()
    assert (pr[one] == 0.0).all() and (cd[one] == 1.0).all()
    assert (cd[y == e] == 1.0).all() and (cd[y != e] < 1.0).all()
    assert (pr[x == a] == 0.0).all() and (pr[x != a] > 0.0).all()
    assert (pr <= 1.0).all() and (cd > 0.0).all()


@pytest.mark.gpu
def test_independent_of_neighbours(gdk):
    m = 300_001
    r = rng(9)
    o_in = (r.random(m) < 0.05).astype(np.int8)
    got = {}
    for pre in (5, 70_001, 0):
        n = pre + m + (17 if pre else 0)
        p, o = np.zeros(n, np.int8), (r.random(n) < 0.5).astype(np.int8)
        p[1:pre:3] = 1
        p[pre] = 1
        o[pre:pre + m] = o_in
        if pre:
            p[pre + m] = 1
        b, P, O = rows(gdk, n), bits(gdk, p), bits(gdk, o)
        for fn in FUNCS:
            res = call(gdk, fn, b, P, O)
            same(gdk, res, model(fn, n, p, o), n, 0, (fn, pre))
            got[fn, pre] = res.to_numpy()[pre:pre + m]
    for fn in FUNCS:
        w = got[fn, 0].view(np.uint8)
        assert np.array_equal(got[fn, 5].view(np.uint8), w), fn
        assert np.array_equal(got[fn, 70_001].view(np.uint8), w), fn


@pytest.mark.gpu
def test_views_and_longer_bits(gdk):
    """p / o longer than b, and views that do not start on a 16-byte boundary"""
    n = 50_001
    r = rng(3)
    p = (r.random(n + 40) < 0.01).astype(np.int8)
    o = (r.random(n + 40) < 0.3).astype(np.int8)
    P, O = bits(gdk, p), bits(gdk, o)
    check(gdk, n, p, o, P=P, O=O)
    for lo in (3, 16):
        Pv, Ov = gdk.BATslice(P, lo, lo + n), gdk.BATslice(O, lo, lo + n + 7)
        check(gdk, n, p[lo:lo + n], o[lo:lo + n + 7], P=Pv, O=Ov)


@pytest.mark.gpu
def test_errors(gdk):
    n = 1000
    b = rows(gdk, n)
    short = bits(gdk, np.zeros(n - 1, np.int8))
    ints = gdk.BAT.from_numpy(gdk.TYPE_int, np.zeros(n, np.int32))
    good = bits(gdk, np.zeros(n, np.int8))
    for bad in (short, ints):
        for fn in FUNCS:
            with pytest.raises(gdk.GDKError) as ei:
                call(gdk, fn, b, bad, good)
            assert str(ei.value)
            if fn != "row_number":
                with pytest.raises(gdk.GDKError) as ei:
                    call(gdk, fn, b, good, bad)
                assert str(ei.value)
                with pytest.raises(gdk.GDKError) as ei:
                    call(gdk, fn, b, bad, None)
                assert str(ei.value)
