"""The parallel form of order-dependent float folds over SEVERAL groups or
partitions (mgdk_set_fp_parallel_min; test_fp_parallel.py covers one).

Every group / partition of at least fp_parallel_min candidate rows (nils
included) takes the blocked, pairwise-combined form; the smaller ones of the
same call are replayed and equal the oracle bit for bit.  A large group's
result differs from the sequential fold by rounding only, within the bounds
DESIGN.md 11.5 states, evaluated per group (n the group's value count, the
sums over the group's values, u = 2^-53, 2^-24 for a flt accumulator):

  mean:         |par - seq| <= 4 n u max|x|
  variance:     |par - seq| <= 4 n u sum(x^2) / (n - s)
  stdev:        |par - seq| <= that / (2 stdev) + 2 ulp
  covariance:   |par - seq| <= 4 n u sqrt(sum x^2 sum y^2) / (n - s)
  correlation:  |par - seq| <= 8 n u (kx + ky + kxy)
  running sum:  |par - seq| <= 2 n u sum|x| on every row

A float64 numpy evaluation (pairwise sums) of the same statistic has to lie
inside the same bound of the oracle: the inputs are well conditioned, the
bounds are not vacuous.  The profiler scopes groupavg_fp_seg,
groupstats_fp_seg and analyticalsum_fp_seg run only on the new path, so
their launch counts tell which path a call took."""
import math

import numpy as np
import pytest

from helpers import rng

U = 2.0 ** -53
THR = 1000
I32N = -(1 << 31)
NPT = {"flt": np.float32, "dbl": np.float64, "int": np.int32}
STATS = [("stdev", True), ("stdev", False), ("variance", True), ("variance", False), ("covariance", True),
         ("covariance", False), ("correlation", False)]


@pytest.fixture
def par(gdk):
    prev = gdk.set_fp_parallel_min(THR)
    gdk.prof_enable(True)
    yield
    gdk.prof_enable(False)
    gdk.set_fp_parallel_min(prev)


def _launches(gdk, name, fn):
    """fn()'s result and how often the scope `name` ran in it"""
    gdk.prof_reset()
    r = fn()
    return r, gdk.prof_get(name)[1]


def _xy(seed, n, tname, nan_every=0):
    """x = N(50, 100), y = 0.5 x + noise as float64 (NaN = nil) in tname's values"""
    r = rng(seed)
    x = r.standard_normal(n) * 100.0 + 50.0
    y = 0.5 * x + (r.standard_normal(n) * 100.0 + 50.0) * 0.3
    if tname == "int":
        x, y = np.rint(x), np.rint(y)
    elif tname == "flt":
        x, y = x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)
    if nan_every:
        x[::nan_every] = np.nan
        y[5::nan_every + 96] = np.nan
    return x, y


def _bats(gdk, ora, tname, v):
    if tname == "int":
        a = np.where(np.isnan(v), I32N, v).astype(np.int32)
    else:
        a = v.astype(NPT[tname])
    return (gdk.BAT.from_numpy(getattr(gdk, "TYPE_" + tname), a, sorted_=False, revsorted=False, key=False),
            ora.Bat.from_array(getattr(ora, "TYPE_" + tname), a))


def _gbats(gdk, ora, gid, hseq=0):
    gid = np.asarray(gid, np.uint64)
    return (gdk.BAT.from_numpy(gdk.TYPE_oid, gid, hseqbase=hseq, sorted_=False, revsorted=False, key=False),
            ora.Bat.from_array(ora.TYPE_oid, gid, hseqbase=hseq))


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _gstat(gdk, name, sample, X, Y, G, E, skip, s=None):
    if name in ("stdev", "variance"):
        return getattr(gdk, "BATgroup%s_%s" % (name, "sample" if sample else "population"))(X, G, E, skip, s)
    if name == "covariance":
        return getattr(gdk, "BATgroupcovariance_%s" % ("sample" if sample else "population"))(X, Y, G, E, skip, s)
    return gdk.BATgroupcorrelation(X, Y, G, E, skip, s)


def _mean_bound(xs):
    return 4 * len(xs) * U * float(np.max(np.abs(xs)))


def _stat_bound(name, sample, xs, ys, want):
    """the bound of one group's statistic and a float64 numpy evaluation of it"""
    s = 1 if sample else 0
    n = len(xs)
    sx = float(np.sum(xs * xs))
    dx = xs - xs.mean()
    if name in ("stdev", "variance"):
        vb = 4 * n * U * sx / (n - s)
        v = float(np.sum(dx * dx)) / (n - s)
        if name == "variance":
            return vb, v
        return vb / (2 * want) + 2 * math.ulp(want), math.sqrt(v)
    sy = float(np.sum(ys * ys))
    dy = ys - ys.mean()
    if name == "covariance":
        return 4 * n * U * math.sqrt(sx * sy) / (n - s), float(np.sum(dx * dy)) / (n - s)
    kx, ky = sx / float(np.sum(dx * dx)), sy / float(np.sum(dy * dy))
    kxy = math.sqrt(sx * sy) / abs(float(np.sum(dx * dy)))
    return 8 * n * U * (kx + ky + kxy), float(np.sum(dx * dy)) / math.sqrt(float(np.sum(dx * dx)) * float(np.sum(dy * dy)))


def _check_avg(got, gcnt, want, wcnt, x, gid, groups, large, skip):
    """counts and nils as the oracle's; small groups bit for bit, large ones within the mean's bound"""
    assert np.array_equal(gcnt, wcnt)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    for k in groups:
        if k not in large:
            assert _same(got[k], want[k]), k
        elif not np.isnan(want[k]):
            xs = x[(gid == k) & ~np.isnan(x)]
            assert len(xs) == wcnt[k]
            assert abs(got[k] - want[k]) <= _mean_bound(xs), (k, got[k], want[k])
            assert abs(float(xs.mean()) - want[k]) <= _mean_bound(xs)


def _check_stat(name, sample, got, want, x, y, gid, groups, large):
    assert np.array_equal(np.isnan(got), np.isnan(want)), (name, sample)
    two = name in ("covariance", "correlation")
    for k in groups:
        if k not in large:
            assert _same(got[k], want[k]), (name, sample, k)
        elif not np.isnan(want[k]):
            m = (gid == k) & ~np.isnan(x)
            if two:
                m &= ~np.isnan(y)
            b, ref = _stat_bound(name, sample, x[m], y[m], want[k])
            assert abs(got[k] - want[k]) <= b, (name, sample, k, got[k], want[k])
            assert abs(ref - want[k]) <= b, (name, sample, k)


def _lens(ng):
    """ng group lengths, all >= THR: exactly THR, 4096, 4097, 256 k + 1, 70000 among them"""
    if ng == 2:
        return [4097, 70_000]
    if ng == 4:
        return [THR, 4096, 256 * 13 + 1, 65_537]
    r = rng(1900)
    return [THR, 4096, 4097, 256 * 13 + 1] + [int(v) for v in r.integers(3000, 4600, ng - 4)]


def _interleaved(ng):
    lens = _lens(ng)
    gid = np.repeat(np.arange(ng, dtype=np.uint64), lens)
    return rng(1901 + ng).permutation(gid)


# ---- 1: every group large --------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("ng", [2, 4, 64])
@pytest.mark.parametrize("tname", ["flt", "dbl"])
@pytest.mark.parametrize("skip", [True, False])
def test_gpu_groupavg_all_large(gdk, ora, par, ng, tname, skip):
    gid = _interleaved(ng)
    x, _ = _xy(1910 + ng, len(gid), tname, nan_every=211)
    (X, OX), (G, OG) = _bats(gdk, ora, tname, x), _gbats(gdk, ora, gid)
    (a, c), runs = _launches(gdk, "groupavg_fp_seg", lambda: gdk.BATgroupavg(X, G, gdk.BAT.dense(0, ng), skip))
    oa, oc = ora.BATgroupavg(OX, OG, ora.Bat.dense(0, ng), skip)
    assert runs == 1
    got, want = a.to_numpy(), np.asarray(oa.values())
    _check_avg(got, c.to_numpy(), want, np.asarray(oc.values()), x, gid, range(ng), set(range(ng)), skip)
    assert (bool(a.s.tnil), bool(a.s.tnonil)) == (bool(oa.s.nil), bool(oa.s.nonil))


@pytest.mark.gpu
@pytest.mark.parametrize("ng", [2, 4, 64])
@pytest.mark.parametrize("tname", ["dbl", "flt", "int"])
@pytest.mark.parametrize("skip", [True, False])
def test_gpu_groupstats_all_large(gdk, ora, par, ng, tname, skip):
    gid = _interleaved(ng)
    x, y = _xy(1920 + ng, len(gid), tname, nan_every=211)
    (X, OX), (Y, OY), (G, OG) = _bats(gdk, ora, tname, x), _bats(gdk, ora, tname, y), _gbats(gdk, ora, gid)
    E, OE = gdk.BAT.dense(0, ng), ora.Bat.dense(0, ng)
    for name, sample in STATS:
        two = name in ("covariance", "correlation")
        r, runs = _launches(gdk, "groupstats_fp_seg", lambda: _gstat(gdk, name, sample, X, Y, G, E, skip))
        o = ora.BATgroupstat(name, OX, OY if two else None, OG, OE, skip, None, sample)
        assert runs == 1, (name, sample)
        _check_stat(name, sample, r.to_numpy(), np.asarray(o.values(), np.float64), x, y, gid, range(ng),
                    set(range(ng)))
        assert (bool(r.s.tnil), bool(r.s.tnonil)) == (bool(o.s.nil), bool(o.s.nonil)), (name, sample)


# ---- 2: large groups among many small ones ----------------------------------

def _mixed():
    """504 groups: 500 of 1..999 rows, an empty one, the large ones A (nils
    inside), B, C and D (nothing but nils); rows of ids beyond e's range"""
    r = rng(1930)
    ng = 505
    lens = r.integers(1, THR, ng)
    large = {3: THR, 250: 5000, 504: 20_000, 77: 1500}      # A = 250, D = 77
    for k, ln in large.items():
        lens[k] = ln
    lens[100] = 0
    lens[101] = THR - 1
    gid = np.repeat(np.arange(ng, dtype=np.uint64), lens)
    gid = np.concatenate([gid, np.full(700, ng + 5, np.uint64), np.full(1200, ng, np.uint64)])
    gid = r.permutation(gid)
    x, y = _xy(1931, len(gid), "dbl")
    small = ~np.isin(gid, list(large))
    x[small & (r.random(len(gid)) < 0.01)] = np.nan
    a = np.flatnonzero(gid == 250)
    x[a[::97]] = np.nan
    x[gid == 77] = np.nan
    return ng, gid, x, y, set(large)


@pytest.mark.gpu
@pytest.mark.parametrize("skip", [True, False])
def test_gpu_mixed_groups(gdk, ora, par, skip):
    ng, gid, x, y, large = _mixed()
    (X, OX), (Y, OY), (G, OG) = _bats(gdk, ora, "dbl", x), _bats(gdk, ora, "dbl", y), _gbats(gdk, ora, gid)
    E, OE = gdk.BAT.dense(0, ng), ora.Bat.dense(0, ng)
    (a, c), runs = _launches(gdk, "groupavg_fp_seg", lambda: gdk.BATgroupavg(X, G, E, skip))
    oa, oc = ora.BATgroupavg(OX, OG, OE, skip)
    assert runs == 1
    got, want = a.to_numpy(), np.asarray(oa.values())
    _check_avg(got, c.to_numpy(), want, np.asarray(oc.values()), x, gid, range(ng), large, skip)
    assert np.isnan(got[100]) and np.isnan(got[77])
    # without skip_nils the one valued large group holding a nil is nil, the others are not
    assert np.isnan(got[250]) == (not skip) and not np.isnan(got[[3, 504]]).any()
    for name, sample in STATS:
        two = name in ("covariance", "correlation")
        r, runs = _launches(gdk, "groupstats_fp_seg", lambda: _gstat(gdk, name, sample, X, Y, G, E, skip))
        o = ora.BATgroupstat(name, OX, OY if two else None, OG, OE, skip, None, sample)
        assert runs == 1, (name, sample)
        got = r.to_numpy()
        _check_stat(name, sample, got, np.asarray(o.values(), np.float64), x, y, gid, range(ng), large)
        assert np.isnan(got[250]) == (not skip) and not np.isnan(got[[3, 504]]).any()
        assert (bool(r.s.tnil), bool(r.s.tnonil)) == (bool(o.s.nil), bool(o.s.nonil))


# ---- 3: the threshold -------------------------------------------------------

@pytest.mark.gpu
def test_gpu_threshold_edge(gdk, ora, par):
    gid = rng(1940).permutation(np.repeat(np.arange(2, dtype=np.uint64), [THR - 1, THR]))
    x, y = _xy(1941, len(gid), "dbl", nan_every=211)
    (X, OX), (G, OG) = _bats(gdk, ora, "dbl", x), _gbats(gdk, ora, gid)
    E, OE = gdk.BAT.dense(0, 2), ora.Bat.dense(0, 2)
    oa, oc = ora.BATgroupavg(OX, OG, OE, True)
    ov = np.asarray(ora.BATgroupstat("variance", OX, None, OG, OE, True, None, True).values(), np.float64)
    want, wcnt = np.asarray(oa.values()), np.asarray(oc.values())

    (a, c), runs = _launches(gdk, "groupavg_fp_seg", lambda: gdk.BATgroupavg(X, G, E, True))
    assert runs == 1
    _check_avg(a.to_numpy(), c.to_numpy(), want, wcnt, x, gid, range(2), {1}, True)
    v, runs = _launches(gdk, "groupstats_fp_seg", lambda: gdk.BATgroupvariance_sample(X, G, E, True))
    assert runs == 1
    _check_stat("variance", True, v.to_numpy(), ov, x, y, gid, range(2), {1})

    # the knob at "never": the replay everywhere
    prev = gdk.set_fp_parallel_min(None)
    try:
        (a, c), runs = _launches(gdk, "groupavg_fp_seg", lambda: gdk.BATgroupavg(X, G, E, True))
        v, runs2 = _launches(gdk, "groupstats_fp_seg", lambda: gdk.BATgroupvariance_sample(X, G, E, True))
    finally:
        gdk.set_fp_parallel_min(prev)
    assert runs == 0 and runs2 == 0
    assert _same(a.to_numpy(), want) and np.array_equal(c.to_numpy(), wcnt) and _same(v.to_numpy(), ov)

    # no group reaches the threshold: the replay everywhere
    gid2 = rng(1942).permutation(np.repeat(np.arange(3, dtype=np.uint64), [THR - 1, THR - 1, 400]))
    x2, _ = _xy(1943, len(gid2), "dbl", nan_every=211)
    (X2, OX2), (G2, OG2) = _bats(gdk, ora, "dbl", x2), _gbats(gdk, ora, gid2)
    (a, c), runs = _launches(gdk, "groupavg_fp_seg", lambda: gdk.BATgroupavg(X2, G2, gdk.BAT.dense(0, 3), True))
    v, runs2 = _launches(gdk, "groupstats_fp_seg",
                         lambda: gdk.BATgroupvariance_sample(X2, G2, gdk.BAT.dense(0, 3), True))
    assert runs == 0 and runs2 == 0
    oa, oc = ora.BATgroupavg(OX2, OG2, ora.Bat.dense(0, 3), True)
    assert _same(a.to_numpy(), oa.values()) and np.array_equal(c.to_numpy(), oc.values())
    assert _same(v.to_numpy(), ora.BATgroupstat("variance", OX2, None, OG2, ora.Bat.dense(0, 3), True, None,
                                                True).values())


# ---- 4: candidates ---------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("cand", ["oids", "dense"])
def test_gpu_candidates(gdk, ora, par, cand):
    """a group is large by its candidate rows: group 0 has 2400 rows but about
    800 candidates and is replayed, group 1 is large, group 2 is small"""
    r = rng(1950)
    n = 90_000
    gid = r.permutation(np.repeat(np.arange(3, dtype=np.uint64), [2400, n - 2400 - 300, 300]))
    x, y = _xy(1951, n, "dbl", nan_every=211)
    if cand == "oids":
        sel = np.sort(r.choice(n, n // 3, replace=False))
        S = gdk.BAT.from_numpy(gdk.TYPE_oid, sel.astype(np.uint64), sorted_=True, key=True, nonil=True)
        OS = ora.Bat.from_array(ora.TYPE_oid, sel.astype(np.uint64), sorted_=True, key=True, nonil=True)
    else:
        sel = np.arange(1000, 1000 + n // 3)
        S, OS = gdk.BAT.dense(1000, len(sel)), ora.Bat.dense(1000, len(sel))
    assert np.sum(gid[sel] == 0) < THR <= np.sum(gid[sel] == 1)
    (X, OX), (Y, OY) = _bats(gdk, ora, "dbl", x), _bats(gdk, ora, "dbl", y)
    G, OG = _gbats(gdk, ora, gid[sel], hseq=int(sel[0]))
    E, OE = gdk.BAT.dense(0, 3), ora.Bat.dense(0, 3)
    (a, c), runs = _launches(gdk, "groupavg_fp_seg", lambda: gdk.BATgroupavg(X, G, E, True, s=S))
    oa, oc = ora.BATgroupavg(OX, OG, OE, True, s=OS)
    assert runs == 1
    _check_avg(a.to_numpy(), c.to_numpy(), np.asarray(oa.values()), np.asarray(oc.values()), x[sel], gid[sel],
               range(3), {1}, True)
    for name, sample in (("variance", True), ("correlation", False)):
        two = name == "correlation"
        v, runs = _launches(gdk, "groupstats_fp_seg", lambda: _gstat(gdk, name, sample, X, Y, G, E, True, S))
        o = ora.BATgroupstat(name, OX, OY if two else None, OG, OE, True, OS, sample)
        assert runs == 1
        _check_stat(name, sample, v.to_numpy(), np.asarray(o.values(), np.float64), x[sel], y[sel], gid[sel],
                    range(3), {1})


# ---- 5: a large group's result does not depend on the layout --------------------

@pytest.mark.gpu
def test_gpu_layout_independence(gdk, par):
    """the same values in the same candidate order: as one of 2 contiguous
    groups, and interleaved row by row among 64 groups"""
    m = 9001
    x, _ = _xy(1960, m, "dbl", nan_every=211)
    other, _ = _xy(1961, 64 * m, "dbl")
    # layout 1: [x | 5000 other rows], groups 0 and 1
    v1 = np.concatenate([x, other[:5000]])
    g1 = np.repeat(np.arange(2, dtype=np.uint64), [m, 5000])
    # layout 2: row i of x at position 64 i + 17, the 63 other groups around it
    v2 = other.copy()
    v2[17::64] = x
    g2 = np.tile(np.arange(64, dtype=np.uint64), m)
    res = []
    for v, g, ng, k in ((v1, g1, 2, 0), (v2, g2, 64, 17), (v2, g2, 64, 17)):
        X = gdk.BAT.from_numpy(gdk.TYPE_dbl, v, sorted_=False, revsorted=False, key=False)
        G = gdk.BAT.from_numpy(gdk.TYPE_oid, g, sorted_=False, revsorted=False, key=False)
        E = gdk.BAT.dense(0, ng)
        (a, c), runs = _launches(gdk, "groupavg_fp_seg", lambda: gdk.BATgroupavg(X, G, E, True))
        var, runs2 = _launches(gdk, "groupstats_fp_seg", lambda: gdk.BATgroupvariance_sample(X, G, E, True))
        assert runs == 1 and runs2 == 1
        res.append((a.to_numpy()[k].tobytes(), int(c.to_numpy()[k]), var.to_numpy()[k].tobytes()))
    assert res[0] == res[1] == res[2]


# ---- 6: grouped moments with a single group ------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("skip", [True, False])
def test_gpu_groupstats_one_group(gdk, ora, par, skip):
    n = 50_000
    x, y = _xy(1970, n, "dbl", nan_every=211 if skip else 0)
    gid = np.zeros(n, np.uint64)
    gid[::1000] = 1                    # rows outside the group range [0, 1)
    (X, OX), (Y, OY), (G, OG) = _bats(gdk, ora, "dbl", x), _bats(gdk, ora, "dbl", y), _gbats(gdk, ora, gid)
    E, OE = gdk.BAT.dense(0, 1), ora.Bat.dense(0, 1)
    for name, sample in STATS:
        two = name in ("covariance", "correlation")
        r, runs = _launches(gdk, "groupstats_fp_seg", lambda: _gstat(gdk, name, sample, X, Y, G, E, skip))
        o = ora.BATgroupstat(name, OX, OY if two else None, OG, OE, skip, None, sample)
        assert runs == 1, (name, sample)
        got = r.to_numpy()
        assert not np.isnan(got[0])
        _check_stat(name, sample, got, np.asarray(o.values(), np.float64), x, y, gid, range(1), {0})
    if not skip:
        x[4321] = np.nan
        X, _ = _bats(gdk, ora, "dbl", x)
        r = gdk.BATgroupvariance_sample(X, G, E, False)
        assert np.isnan(r.to_numpy()[0]) and r.s.tnil


# ---- 7: overflow -----------------------------------------------------------

@pytest.mark.gpu
def test_gpu_groupstats_overflow(gdk, par):
    x, _ = _xy(1980, 9000, "dbl")
    gid = rng(1981).permutation(np.repeat(np.arange(3, dtype=np.uint64), [3000, 5000, 1000]))
    big = np.flatnonzero(gid == 1)
    x[big[::2]] = 1e300
    x[big[1::2]] = -1e300
    X = gdk.BAT.from_numpy(gdk.TYPE_dbl, x, sorted_=False, revsorted=False, key=False)
    G = gdk.BAT.from_numpy(gdk.TYPE_oid, gid, sorted_=False, revsorted=False, key=False)
    with pytest.raises(gdk.GDKError, match="overflow in calculation"):
        gdk.BATgroupvariance_population(X, G, gdk.BAT.dense(0, 3), True)


# ---- 8: the running sum over several partitions ----------------------------------

def _peers(r, n, maxrun):
    o = np.zeros(n, np.int8)
    i = 0
    while i < n:
        o[i] = 1
        i += int(r.integers(1, maxrun + 1))
    return o


def _partitions(nlarge):
    """partition lengths: nlarge of >= THR rows (4096 and 4097 among them) with small ones between"""
    r = rng(1990 + nlarge)
    if nlarge == 2:
        large = [4097, 60_000]
    elif nlarge == 4:
        large = [4096, THR, 30_000, 4097]
    else:
        large = [4096, 4097, THR] + [int(v) for v in r.integers(1500, 4500, nlarge - 3)]
    lens, islarge = [], []
    for i, ln in enumerate(large):
        if i % 3 == 0:
            lens.append(int(r.integers(1, THR)))
            islarge.append(False)
        lens.append(ln)
        islarge.append(True)
    lens += [THR - 1, 1]
    islarge += [False, False]
    return lens, islarge


@pytest.mark.gpu
@pytest.mark.parametrize("frame", [3, 4])
@pytest.mark.parametrize("types", [("dbl", "dbl"), ("flt", "dbl"), ("flt", "flt")])
@pytest.mark.parametrize("nlarge,maxrun", [(2, 9000), (4, 1), (4, 0), (64, 50)])
def test_gpu_running_sum_partitions(gdk, ora, par, frame, types, nlarge, maxrun):
    lens, islarge = _partitions(nlarge)
    starts = np.concatenate([[0], np.cumsum(lens)])
    n = int(starts[-1])
    r = rng(1995 + maxrun)
    x = r.standard_normal(n) * 10.0
    x[starts[1]:starts[1] + 37] = np.nan     # leading nils of the first large partition
    x[starts[-3] + 5] = np.nan               # and a nil inside a small one
    x[::997] = np.nan
    t1, t2 = types
    if t1 == "flt":
        x = x.astype(np.float32)
    p = np.zeros(n, np.int8)
    p[starts[:-1]] = 1
    if maxrun:
        o = _peers(r, n, maxrun) | p
    else:
        o = p.copy()                         # one peer run per partition
    tp1, tp2 = getattr(gdk, "TYPE_" + t1), getattr(gdk, "TYPE_" + t2)
    res, runs = _launches(gdk, "analyticalsum_fp_seg", lambda: gdk.GDKanalyticalsum(
        gdk.BAT.from_numpy(tp1, x), gdk.BAT.from_numpy(gdk.TYPE_bit, p), gdk.BAT.from_numpy(gdk.TYPE_bit, o), None,
        None, tp2, frame))
    assert runs == 1
    got = res.to_numpy().astype(np.float64)
    ores = ora.analyticalsum(ora.Bat.from_array(getattr(ora, "TYPE_" + t1), x), ora.Bat.from_array(ora.TYPE_bit, p),
                             ora.Bat.from_array(ora.TYPE_bit, o), None, None, getattr(ora, "TYPE_" + t2), frame)
    want = np.asarray(ores.values()).astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert (bool(res.s.tnil), bool(res.s.tnonil)) == (bool(ores.s.nil), bool(ores.s.nonil))
    u = 2.0 ** -24 if t2 == "flt" else U
    xd = x.astype(np.float64)
    for k, big in enumerate(islarge):
        a, b = int(starts[k]), int(starts[k + 1])
        if not big:
            assert _same(got[a:b], want[a:b]), k
            continue
        bound = 2 * (b - a) * u * float(np.nansum(np.abs(xd[a:b])))
        d = np.nan_to_num(np.abs(got[a:b] - want[a:b]))
        assert float(d.max()) <= bound, (k, float(d.max()), bound)
        # a float64 evaluation of the same running sum lies inside the bound too
        if t2 == "dbl" and maxrun == 1:
            seq = np.nancumsum(xd[a:b] if frame == 3 else xd[a:b][::-1])
            ref = seq if frame == 3 else seq[::-1]
            ok = ~np.isnan(want[a:b])
            assert float(np.abs(ref[ok] - want[a:b][ok]).max()) <= bound


@pytest.mark.gpu
def test_gpu_running_sum_partitions_below_threshold(gdk, ora, par):
    """no partition reaches the threshold, and the knob at never: the replay, bit for bit"""
    lens = [THR - 1, 500, THR - 1, 1]
    n = sum(lens)
    x = rng(1997).standard_normal(n) * 10.0
    p = np.zeros(n, np.int8)
    p[np.concatenate([[0], np.cumsum(lens)[:-1]])] = 1
    o = _peers(rng(1998), n, 7) | p
    args = lambda m, mk: (mk(m.TYPE_dbl, x), mk(m.TYPE_bit, p), mk(m.TYPE_bit, o))
    B, P, O = args(gdk, gdk.BAT.from_numpy)
    OB, OP, OO = args(ora, ora.Bat.from_array)
    want = np.asarray(ora.analyticalsum(OB, OP, OO, None, None, ora.TYPE_dbl, 3).values())
    res, runs = _launches(gdk, "analyticalsum_fp_seg",
                          lambda: gdk.GDKanalyticalsum(B, P, O, None, None, gdk.TYPE_dbl, 3))
    assert runs == 0 and _same(res.to_numpy(), want)
    lens2, _ = _partitions(2)
    n2 = sum(lens2)
    x2 = rng(1999).standard_normal(n2) * 10.0
    p2 = np.zeros(n2, np.int8)
    p2[np.concatenate([[0], np.cumsum(lens2)[:-1]])] = 1
    prev = gdk.set_fp_parallel_min(None)
    try:
        res, runs = _launches(gdk, "analyticalsum_fp_seg", lambda: gdk.GDKanalyticalsum(
            gdk.BAT.from_numpy(gdk.TYPE_dbl, x2), gdk.BAT.from_numpy(gdk.TYPE_bit, p2),
            gdk.BAT.from_numpy(gdk.TYPE_bit, p2), None, None, gdk.TYPE_dbl, 4))
    finally:
        gdk.set_fp_parallel_min(prev)
    want = np.asarray(ora.analyticalsum(ora.Bat.from_array(ora.TYPE_dbl, x2), ora.Bat.from_array(ora.TYPE_bit, p2),
                                        ora.Bat.from_array(ora.TYPE_bit, p2), None, None, ora.TYPE_dbl, 4).values())
    assert runs == 0 and _same(res.to_numpy(), want)


@pytest.mark.gpu
def test_gpu_running_sum_partitions_overflow(gdk, par):
    lens = [300, 10_000, 2000]
    n = sum(lens)
    x = rng(2000).standard_normal(n)
    x[300:10_300] = 1e308
    p = np.zeros(n, np.int8)
    p[[0, 300, 10_300]] = 1
    o = np.ones(n, np.int8)
    with pytest.raises(gdk.GDKError, match="overflow"):
        gdk.GDKanalyticalsum(gdk.BAT.from_numpy(gdk.TYPE_dbl, x), gdk.BAT.from_numpy(gdk.TYPE_bit, p),
                             gdk.BAT.from_numpy(gdk.TYPE_bit, o), None, None, gdk.TYPE_dbl, 3)
