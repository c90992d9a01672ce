"""The parallel form of the windowed float AVG and the window statistics
(mgdk_set_fp_parallel_min; test_fp_parallel_groups.py covers the grouped
folds and the running SUM).

GDKanalyticalavg of flt / dbl (frames 3, 5) and the seven GDKanalytical_*
statistics (frames 3, 4, 5, every input type) run every partition of at least
fp_parallel_min rows (nils included) as a blocked scan of pairwise-combined
states; the smaller partitions of the same call are replayed and equal the
oracle bit for bit.  A row of a large partition differs from the sequential
fold by rounding only, within DESIGN.md 11.5's bounds applied to the row's
fold prefix (k its non-nil values xs, ys: frame 3 the partition start through
the end of the row's peer run, frame 4 the partition end back through the
start of its run, frame 5 the partition; s = 1 for sample forms; U = 2^-53,
u = 2^-24 for AVG of flt, else U):

  AVG:          |par - seq| <= 4 k u max|xs|
  variance:     |par - seq| <= 4 k U sum(xs^2) / (k - s)
  stdev:        |par - seq| <= that / (2 stdev) + 2 ulp
  covariance:   |par - seq| <= 4 k U sqrt(sum xs^2 sum ys^2) / (k - s)
  correlation:  |par - seq| <= 8 k U (kx + ky + kxy)

Rows whose bound is not finite (no spread yet, k <= s) are skipped and are
under 1 % of the large partitions' rows.  A float64 numpy evaluation from
prefix sums lies inside the same bound of the oracle, so the bounds are not
vacuous.  The profiler scopes analyticalavg_fp_seg and analytic_stats_fp_seg
run only on the new path, so their launch counts tell which path a call took."""
import functools

import numpy as np
import pytest

from helpers import rng

U = 2.0 ** -53
THR = 1000
I32N = -(1 << 31)
NPT = {"flt": np.float32, "dbl": np.float64, "int": np.int32}
STATS = ["stddev_samp", "stddev_pop", "variance_samp", "variance_pop", "covariance_samp", "covariance_pop",
         "correlation"]
AVG_SCOPE, STAT_SCOPE = "analyticalavg_fp_seg", "analytic_stats_fp_seg"


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


def _xy(seed, n, tname, nan_every=211):
    """x = N(50, 100), y = 0.5 x + noise as float64 (NaN = nil) in tname's values"""
    r = rng(seed)
    x = r.standard_normal(n) * 100.0 + 50.0
    y = 0.5 * x + (r.standard_normal(n) * 100.0 + 50.0) * 0.3
    if tname in ("int", "hge"):
        x, y = np.rint(x), np.rint(y)
    elif tname == "flt":
        x, y = x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)
    if nan_every:
        x[::nan_every] = np.nan
        y[5::nan_every + 96] = np.nan
    return x, y


def _arr(tname, v):
    """the column of tname holding the float64 values v (NaN = nil)"""
    if tname == "int":
        return np.where(np.isnan(v), I32N, v).astype(np.int32)
    if tname == "hge":
        i = np.where(np.isnan(v), 0, v).astype(np.int64)
        w = np.empty((len(v), 2), np.uint64)
        w[:, 0] = i.view(np.uint64)
        w[:, 1] = np.where(i < 0, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0))
        w[np.isnan(v), 0] = 0
        w[np.isnan(v), 1] = np.uint64(1 << 63)
        return w
    return v.astype(NPT[tname])


def _bats(gdk, ora, tname, v):
    a = _arr(tname, v)
    return (gdk.BAT.from_numpy(getattr(gdk, "TYPE_" + tname), a), ora.Bat.from_array(getattr(ora, "TYPE_" + tname), a))


def _bits(gdk, ora, b):
    if b is None:
        return None, None
    return gdk.BAT.from_numpy(gdk.TYPE_bit, b), ora.Bat.from_array(ora.TYPE_bit, b)


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _peers(r, n, maxrun):
    o = np.zeros(n, np.int8)
    i = 0
    while i < n:
        o[i] = 1
        i += int(r.integers(1, maxrun + 1))
    return o


LAYOUTS = {
    "edges": [8229, 999, 1000, 4096, 4097, 300],
    "four": [17, 2500, 400, 2500, 999, 2500, 3, 2500, 250],
    "many": sum(([1100] * 4 + [37 + 3 * i] for i in range(16)), []),
}


class Layout:
    """partition lengths -> starts, the partition bits p and random peer bits o"""

    def __init__(self, lens, seed=2100, maxrun=7, o=None):
        self.lens = [int(v) for v in lens]
        self.starts = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.n = int(self.starts[-1])
        self.p = np.zeros(self.n, np.int8)
        self.p[self.starts[:-1]] = 1
        self.o = (_peers(rng(seed), self.n, maxrun) | self.p) if o is None else (o | self.p)
        self.large = [ln >= THR for ln in self.lens]

    def parts(self):
        for k, big in enumerate(self.large):
            yield int(self.starts[k]), int(self.starts[k + 1]), big


@functools.lru_cache(maxsize=None)
def _layout(name):
    return Layout(LAYOUTS[name])


def _prefix(lay, x, y, frame, two):
    """per row of the large partitions (NaN elsewhere): the count and the sums
    over the non-nil values of the row's fold prefix"""
    names = ("k", "sx", "sy", "sxx", "syy", "sxy", "mx")
    out = {nm: np.full(lay.n, np.nan) for nm in names}
    for a, b, big in lay.parts():
        if not big:
            continue
        ln = b - a
        rows = np.arange(a, b) if frame != 4 else np.arange(b - 1, a - 1, -1)      # fold order
        xs, ys = x[rows], (y[rows] if two else np.zeros(ln))
        ok = ~np.isnan(xs) & ~np.isnan(ys)
        xs, ys = np.where(ok, xs, 0.0), np.where(ok, ys, 0.0)
        if frame == 3:
            end = np.r_[lay.o[a + 1:b] != 0, True]
        elif frame == 4:
            end = np.r_[lay.o[rows[:-1]] != 0, True]
        else:
            end = np.r_[np.zeros(ln - 1, bool), True]
        idx = np.where(end, np.arange(ln), ln)
        at = np.minimum.accumulate(idx[::-1])[::-1]           # the end of each position's run
        cols = (ok.astype(np.float64), xs, ys, xs * xs, ys * ys, xs * ys)
        for nm, c in zip(names, cols):
            out[nm][rows] = np.cumsum(c)[at]
        out["mx"][rows] = np.maximum.accumulate(np.abs(xs))[at]
    return out


def _bound(pre, func, want, u=U):
    """the bound per row and the float64 numpy evaluation (both NaN / inf where there is none)"""
    k, sx, sy, sxx, syy, sxy = (pre[nm] for nm in ("k", "sx", "sy", "sxx", "syy", "sxy"))
    with np.errstate(all="ignore"):
        if func == "avg":
            return 4 * k * u * pre["mx"], sx / k
        s = 1.0 if func.endswith("samp") else 0.0
        dxx, dyy, dxy = sxx - sx * sx / k, syy - sy * sy / k, sxy - sx * sy / k
        if func.startswith("variance") or func.startswith("stddev"):
            vb, v = 4 * k * U * sxx / (k - s), dxx / (k - s)
            if func.startswith("variance"):
                return vb, v
            return vb / (2 * want) + 2 * np.spacing(np.abs(want)), np.sqrt(v)
        if func.startswith("covariance"):
            return 4 * k * U * np.sqrt(sxx * syy) / (k - s), dxy / (k - s)
        kx, ky, kxy = sxx / dxx, syy / dyy, np.sqrt(sxx * syy) / np.abs(dxy)
        return 8 * k * U * (kx + ky + kxy), dxy / np.sqrt(dxx * dyy)


def _check(lay, func, frame, got, want, x, y, u=U, skipped_max=0.01):
    """small partitions bit for bit; large ones: the oracle's nils and every row within its bound"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape == (lay.n,)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (func, frame)
    two = func.startswith("cov") or func == "correlation"
    big = np.zeros(lay.n, bool)
    for a, b, isbig in lay.parts():
        if isbig:
            big[a:b] = True
        else:
            assert _same(got[a:b], want[a:b]), (func, frame, a)
    if not big.any():
        return
    bound, ref = _bound(_prefix(lay, x, y, frame, two), func, want, u)
    use = big & np.isfinite(bound) & ~np.isnan(want)
    assert np.count_nonzero(big & ~use) <= skipped_max * np.count_nonzero(big), (func, frame)
    d = np.abs(got - want)
    bad = np.flatnonzero(use & ~(d <= bound))
    assert bad.size == 0, (func, frame, int(bad[0]), got[bad[0]], want[bad[0]], bound[bad[0]])
    dr = np.abs(ref - want)
    bad = np.flatnonzero(use & ~(dr <= bound))
    assert bad.size == 0, ("numpy", func, frame, int(bad[0]), ref[bad[0]], want[bad[0]], bound[bad[0]])


def _flags(got, want):
    assert (bool(got.s.tnil), bool(got.s.tnonil)) == (bool(want.s.nil), bool(want.s.nonil))


def _run_avg(gdk, ora, lay, tname, frame, x, p="bits", expect=1):
    (B, OB), (P, OP), (O, OO) = _bats(gdk, ora, tname, x), _bits(gdk, ora, lay.p if p == "bits" else None), _bits(
        gdk, ora, lay.o)
    got, runs = _launches(gdk, AVG_SCOPE, lambda: gdk.GDKanalyticalavg(B, P, O, None, None, frame))
    want = ora.analyticalavg(OB, OP, OO, None, None, frame)
    assert runs == expect
    _flags(got, want)
    return got.to_numpy(), np.asarray(want.values(), np.float64)


def _run_stat(gdk, ora, lay, tname, name, frame, x, y, p="bits", expect=1):
    two = name.startswith("cov") or name == "correlation"
    (B, OB), (P, OP), (O, OO) = _bats(gdk, ora, tname, x), _bits(gdk, ora, lay.p if p == "bits" else None), _bits(
        gdk, ora, lay.o)
    B2, OB2 = _bats(gdk, ora, tname, y) if two else (None, None)
    got, runs = _launches(gdk, STAT_SCOPE, lambda: gdk.GDKanalytical_stat(name, B, B2, P, O, None, None, frame))
    want = ora.analyticalstat(name, OB, OB2, OP, OO, None, None, frame)
    assert runs == expect, (name, frame)
    _flags(got, want)
    return got.to_numpy(), np.asarray(want.values(), np.float64)


# ---- 1: the bounds over several partitions ------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("frame", [3, 5])
@pytest.mark.parametrize("tname", ["flt", "dbl"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_gpu_window_avg_partitions(gdk, ora, par, layout, tname, frame):
    lay = _layout(layout)
    x, y = _xy(2110, lay.n, tname)
    got, want = _run_avg(gdk, ora, lay, tname, frame, x)
    _check(lay, "avg", frame, got, want, x, y, u=2.0 ** -24 if tname == "flt" else U)
    if tname == "flt":
        # the average of flt values is a flt value, as the reference's is
        ok = ~np.isnan(got)
        assert np.array_equal(got[ok].astype(np.float32).astype(np.float64), got[ok])


@pytest.mark.gpu
@pytest.mark.parametrize("frame", [3, 4, 5])
@pytest.mark.parametrize("tname", ["int", "flt", "dbl"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_gpu_window_stats_partitions(gdk, ora, par, layout, tname, frame):
    lay = _layout(layout)
    x, y = _xy(2120, lay.n, tname)
    for name in STATS:
        got, want = _run_stat(gdk, ora, lay, tname, name, frame, x, y)
        _check(lay, name, frame, got, want, x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("frame", [3, 4, 5])
def test_gpu_window_stats_hge(gdk, ora, par, frame):
    lay = _layout("edges")
    x, y = _xy(2125, lay.n, "hge")
    for name in ("stddev_samp", "covariance_pop", "correlation"):
        got, want = _run_stat(gdk, ora, lay, "hge", name, frame, x, y)
        _check(lay, name, frame, got, want, x, y)


# ---- 2: peer runs ---------------------------------------------------------------

def _peer_layout(shape):
    lens = [300, 9000, 999, 5000]
    n, a = sum(lens), 300
    o = np.ones(n, np.int8)
    if shape == "start":
        o[:] = 0                         # one run per partition
    elif shape == "straddle":
        o[a + 4091:a + 4101] = 0         # rows 4090 .. 4100 of the partition are one run
    elif shape == "long":
        o[a + 101:a + 8900] = 0          # one run with the whole tile 4096 .. 8191 inside
    return Layout(lens, o=o)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["ones", "start", "straddle", "long"])
def test_gpu_window_peer_runs(gdk, ora, par, shape):
    lay = _peer_layout(shape)
    x, y = _xy(2130, lay.n, "dbl")
    # rows that start no run carry their run's value: the same bytes as the row before
    inrun = lay.o[1:] == 0
    res = [("avg", 3) + _run_avg(gdk, ora, lay, "dbl", 3, x)]
    for name, frame in (("variance_samp", 3), ("variance_samp", 4), ("stddev_pop", 4), ("correlation", 3),
                        ("covariance_samp", 4)):
        res.append((name, frame) + _run_stat(gdk, ora, lay, "dbl", name, frame, x, y))
    for func, frame, got, want in res:
        # (with one run per partition a sample form's skipped rows are whole runs)
        _check(lay, func, frame, got, want, x, y)
        g = got.view(np.uint64)
        assert np.array_equal(g[1:][inrun], g[:-1][inrun]), (func, frame)


# ---- 3: nils --------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_window_leading_nils(gdk, ora, par):
    lay = Layout([300, 9000, 400], o=np.ones(9700, np.int8))
    x, y = _xy(2140, lay.n, "dbl")
    x[300:5300] = np.nan
    for frame in (3, 5):
        got, want = _run_avg(gdk, ora, lay, "dbl", frame, x)
        _check(lay, "avg", frame, got, want, x, y, skipped_max=0.6)
        if frame == 3:
            assert np.isnan(got[300:5300]).all() and not np.isnan(got[5301:9300]).any()
    for name, frame in (("stddev_samp", 3), ("variance_pop", 4), ("correlation", 3), ("covariance_samp", 5)):
        got, want = _run_stat(gdk, ora, lay, "dbl", name, frame, x, y)
        _check(lay, name, frame, got, want, x, y, skipped_max=0.6)
        if frame == 3:
            assert np.isnan(got[300:5300]).all() and not np.isnan(got[5310:9300]).any()
        if frame == 4:
            assert not np.isnan(got[300:9200]).any()


@pytest.mark.gpu
def test_gpu_window_all_nil_partition(gdk, ora, par):
    lay = Layout([300, 5000, 2000])
    x, y = _xy(2150, lay.n, "dbl")
    x[300:5300] = np.nan
    for frame in (3, 5):
        got, want = _run_avg(gdk, ora, lay, "dbl", frame, x)
        _check(lay, "avg", frame, got, want, x, y, skipped_max=0.8)
        assert np.isnan(got[300:5300]).all() and not np.isnan(got[5310:]).any()
    for name, frame in (("variance_samp", 3), ("stddev_pop", 4), ("correlation", 5)):
        got, want = _run_stat(gdk, ora, lay, "dbl", name, frame, x, y)
        _check(lay, name, frame, got, want, x, y, skipped_max=0.8)
        assert np.isnan(got[300:5300]).all()


@pytest.mark.gpu
def test_gpu_window_no_partition_column(gdk, ora, par):
    """p = NULL: the column is one partition"""
    lay = Layout([9001])
    x, y = _xy(2160, lay.n, "flt")
    for frame in (3, 5):
        got, want = _run_avg(gdk, ora, lay, "flt", frame, x, p=None)
        _check(lay, "avg", frame, got, want, x, y, u=2.0 ** -24)
    for name, frame in (("stddev_samp", 3), ("variance_pop", 4), ("covariance_pop", 5), ("correlation", 4)):
        got, want = _run_stat(gdk, ora, lay, "flt", name, frame, x, y, p=None)
        _check(lay, name, frame, got, want, x, y)


# ---- 4: a large partition's result does not depend on the layout -------------------

@pytest.mark.gpu
def test_gpu_window_layout_independence(gdk, par):
    m = 9001
    vals, _ = _xy(2170, m, "dbl")
    peers = _peers(rng(2171), m, 9)
    # partition 0 of 2; partition 17 of 40, starting at a row that is no multiple of 4096
    first = [m, 5000]
    second = [700 + 13 * i for i in range(17)] + [m] + [1500 if i % 5 == 0 else 333 for i in range(22)]
    assert len(second) == 40 and sum(second[:17]) % 4096 != 0
    res = []
    for lens, k in ((first, 0), (second, 17), (second, 17)):
        n, a = sum(lens), sum(lens[:k])
        x, _ = _xy(2172, n, "dbl")
        x[a:a + m] = vals
        o = _peers(rng(2173), n, 5)
        o[a:a + m] = peers
        lay = Layout(lens, o=o)
        B, P, O = (gdk.BAT.from_numpy(gdk.TYPE_dbl, x), gdk.BAT.from_numpy(gdk.TYPE_bit, lay.p),
                   gdk.BAT.from_numpy(gdk.TYPE_bit, lay.o))
        avg, r1 = _launches(gdk, AVG_SCOPE, lambda: gdk.GDKanalyticalavg(B, P, O, None, None, 3))
        v3, r2 = _launches(gdk, STAT_SCOPE,
                           lambda: gdk.GDKanalytical_stat("variance_samp", B, None, P, O, None, None, 3))
        v4, r3 = _launches(gdk, STAT_SCOPE,
                           lambda: gdk.GDKanalytical_stat("variance_samp", B, None, P, O, None, None, 4))
        assert (r1, r2, r3) == (1, 1, 1)
        res.append(tuple(r.to_numpy()[a:a + m].tobytes() for r in (avg, v3, v4)))
    assert res[0] == res[1] == res[2]


# ---- 5: the threshold ---------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_window_threshold(gdk, ora, par):
    lay = Layout([THR - 1, THR])
    x, y = _xy(2180, lay.n, "dbl")
    assert lay.large == [False, True]
    for frame in (3, 5):
        got, want = _run_avg(gdk, ora, lay, "dbl", frame, x)
        _check(lay, "avg", frame, got, want, x, y)
    for frame in (3, 4, 5):
        got, want = _run_stat(gdk, ora, lay, "dbl", "variance_samp", frame, x, y)
        _check(lay, "variance_samp", frame, got, want, x, y)

    # the knob at "never": the replay everywhere
    big = _layout("edges")
    xb, yb = _xy(2181, big.n, "dbl")
    prev = gdk.set_fp_parallel_min(None)
    try:
        for frame in (3, 5):
            got, want = _run_avg(gdk, ora, big, "dbl", frame, xb, expect=0)
            assert _same(got, want)
        for name, frame in (("stddev_samp", 3), ("correlation", 4), ("covariance_pop", 5)):
            got, want = _run_stat(gdk, ora, big, "dbl", name, frame, xb, yb, expect=0)
            assert _same(got, want)
    finally:
        gdk.set_fp_parallel_min(prev)

    # no partition reaches the threshold: the replay everywhere
    low = Layout([THR - 1, 500, THR - 1, 1])
    xl, yl = _xy(2182, low.n, "dbl")
    for frame in (3, 5):
        got, want = _run_avg(gdk, ora, low, "dbl", frame, xl, expect=0)
        assert _same(got, want)
    for name, frame in (("stddev_samp", 3), ("correlation", 4), ("covariance_pop", 5)):
        got, want = _run_stat(gdk, ora, low, "dbl", name, frame, xl, yl, expect=0)
        assert _same(got, want)


# ---- 6: overflow ----------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("where", ["large", "small"])
@pytest.mark.parametrize("frame", [3, 4, 5])
def test_gpu_window_stats_overflow(gdk, ora, par, where, frame):
    """an accumulator that leaves the dbl range: in a large partition, and in a
    small one beside a large benign one"""
    lay = Layout([300, 5000, 600])
    x, _ = _xy(2190, lay.n, "dbl", nan_every=0)
    a, b = (300, 5300) if where == "large" else (5300, 5900)
    x[a:b:2] = 1e200
    x[a + 1:b:2] = -1e200
    (B, OB), (P, OP), (O, OO) = _bats(gdk, ora, "dbl", x), _bits(gdk, ora, lay.p), _bits(gdk, ora, lay.o)
    with pytest.raises(ora.OracleError):
        ora.analyticalstat("variance_samp", OB, None, OP, OO, None, None, frame)
    with pytest.raises(gdk.GDKError, match="overflow in calculation"):
        gdk.GDKanalytical_stat("variance_samp", B, None, P, O, None, None, frame)


# ---- 7: frame 4 of the float average stays all nil ---------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("tname", ["flt", "dbl"])
def test_gpu_window_avg_frame4_nil(gdk, ora, par, tname):
    lay = _layout("edges")
    x, _ = _xy(2195, lay.n, tname)
    got, want = _run_avg(gdk, ora, lay, tname, 4, x, expect=0)
    assert np.isnan(got).all() and np.isnan(want).all()
