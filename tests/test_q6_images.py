"""The fused Q6 over column images (Priv::cimg): discount and
quantity read as 1- or 2-byte frame-of-reference codes by the image variants
(24 / 25) of k_q6s.  Every revenue is compared with `==`: with the oracle's
ora.q6 wherever the query has its standard bounds (5 <= discount <= 7,
quantity < 2400, shipdate in 1994), and, where a case needs other bounds
than ora.q6 takes, with an exact Python-integer restatement of the same
predicate, which is itself checked against ora.q6 at the standard bounds.

Sizes: at q6_set_variant(v, 1) the grid is 256 workgroups = 1024 waves of
one 256-row chunk each, so n = 256 * (U * 1024 + 512) + 77 rows runs all
three regions of the kernel: one pass of the loop unrolled U times on every
wave, one left-over chunk on the first 512 waves, and 77 tail rows.  U = 2
for variants 19 / 24 (N2), U = 4 for variants 20 / 25 (N4).  This also pins
the unrolled loop of the raw cascade (19 / 20), which the older
test_q6_variants never reaches: its largest column has fewer chunks than the
16384 waves of its launches, so only the left-over loop runs there.
"""
import functools
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N2 = 256 * (2 * 1024 + 512) + 77     # 655,437
N4 = 256 * (4 * 1024 + 512) + 77     # 1,179,725
IMG, IMG4 = 24, 25                   # the image variants (2 / 4 chunks in flight)
NIL32, NIL64 = np.iinfo(np.int32).min, np.iinfo(np.int64).min
COLS = ("shipdate", "discount", "quantity", "extendedprice")
I64MAX = np.iinfo(np.int64).max


@functools.lru_cache(maxsize=None)
def _gen(n, nils):
    """Generator columns (shared, read-only), with 1 % nils in all four
    columns as test_q6_variants makes them."""
    from oracle import pyoracle as ora
    host = ora.tpch_lineitem(17, 0, n, 20_000)
    host = {k: host[k] for k in COLS + ("tax", "returnflag", "linestatus")}
    if nils:
        r = np.random.default_rng(61)
        for k in COLS:
            host[k][r.random(n) < 0.01] = NIL32 if k == "shipdate" else NIL64
    for v in host.values():
        v.setflags(write=False)
    return host


def host_cols(n, nils=True, **changed):
    h = dict(_gen(n, nils))
    h.update(changed)
    return h


def upload(gdk, host):
    return {k: gdk.BAT.from_numpy(gdk.TYPE_int if k == "shipdate" else gdk.TYPE_lng, host[k]) for k in COLS}


def run_q6(gdk, ora, cols, dlo=5, dhi=7, qmax=2400):
    d0, d1 = ora.mkdate(1994, 1, 1), ora.mkdate(1995, 1, 1)
    return gdk.q6_fused(cols["shipdate"], cols["discount"], cols["quantity"], cols["extendedprice"],
                        d0, d1, dlo, dhi, qmax)


def ora_q6(ora, host, threads=4):
    """ora.q6 on the four Q6 columns of `host` (the oracle's lineitem also
    carries three columns the query does not read)."""
    n = host["shipdate"].shape[0]
    li = {k: np.ascontiguousarray(host[k]) for k in COLS}
    li["tax"] = np.zeros(n, np.int64)
    li["returnflag"] = np.zeros(n, np.uint8)
    li["linestatus"] = np.zeros(n, np.uint8)
    return ora.q6(li, threads)


def model_q6(ora, host, dlo=5, dhi=7, qmax=2400):
    """The raw predicate and the exact sum of products, in Python integers."""
    d0, d1 = ora.mkdate(1994, 1, 1), ora.mkdate(1995, 1, 1)
    sd, di, q, p = (host[k] for k in COLS)
    ok = (sd != NIL32) & (sd >= d0) & (sd < d1) & (di != NIL64) & (q != NIL64) & (p != NIL64)
    if dlo > I64MAX or dhi < NIL64:
        ok &= False
    else:
        ok &= (di >= max(dlo, NIL64)) & (di <= min(dhi, I64MAX))
    ok &= (q < qmax)
    return sum(int(a) * int(b) for a, b in zip(p[ok], di[ok]))


class images:
    """The image variant at `bpc` workgroups per CU, images from 1 row up."""

    def __init__(self, gdk, variant=IMG, bpc=1, min_rows=1):
        self.gdk, self.variant, self.bpc, self.min_rows = gdk, variant, bpc, min_rows

    def __enter__(self):
        self.prev = self.gdk.set_colimg_min(self.min_rows)
        self.gdk.q6_set_variant(self.variant, self.bpc)

    def __exit__(self, *exc):
        self.gdk.q6_set_variant(IMG, 64)
        self.gdk.set_colimg_min(self.prev)


def spread(col, kind, base=0):
    """col (values + nils) moved to `base` and given the spread of an image
    of width 1 (as generated), 2 (one outlier within 65534) or none."""
    out = col.copy()
    live = out != NIL64
    out[live] += base
    first = np.flatnonzero(live)[:2]
    if kind == 2:
        out[first[0]] = out[live].min() - 40_000
    elif kind == 0:
        out[first[0]] = out[live].min() - 40_000
        out[first[1]] = out[live].max() + 40_000
    return out


def narrow_qty(q):
    """quantity squeezed into 2300 .. 2496 (a 1-byte image; about half of it
    below the query's 2400)"""
    out = q.copy()
    live = out != NIL64
    out[live] = 2300 + (out[live] - 100) // 25
    return out


@pytest.mark.parametrize("variant,n,dw,qw",
                         [(IMG, N2, dw, qw) for dw in (1, 2, 0) for qw in (1, 2, 0)] +
                         [(IMG4, N4, 1, 2), (IMG4, N4, 0, 1), (IMG4, N4, 2, 0)])
def test_width_combinations(gdk, ora, variant, n, dw, qw):
    """All nine pairs of image widths (0: ineligible, the column is read raw
    by the same kernel) on nil data with the states colimg_info reports; the
    4-chunk variant runs three of the pairs."""
    g = _gen(n, True)
    host = host_cols(n, discount=spread(g["discount"], dw),
                     quantity=narrow_qty(g["quantity"]) if qw == 1 else spread(g["quantity"], qw))
    cols = upload(gdk, host)
    with images(gdk, variant):
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4)
        for k, w in (("discount", dw), ("quantity", qw)):
            live = host[k][host[k] != NIL64]
            want = (1, w, int(live.min())) if w else (-1, None, None)
            assert gdk.colimg_info(cols[k]) == want, k
        assert gdk.colimg_info(cols["extendedprice"]) == (0, None, None)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_small_columns(gdk, ora, n):
    host = host_cols(n)
    cols = upload(gdk, host)
    with images(gdk):
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 1)
        # a column of nils only has no image
        for k in ("discount", "quantity"):
            if (host[k] != NIL64).any():
                assert gdk.colimg_info(cols[k])[0] == 1


@pytest.mark.parametrize("base", [-3, -(1 << 62) + 11, (1 << 62) - 5000])
def test_bases(gdk, ora, base):
    """Negative bases and bases near +-2^62: the product takes base + code."""
    g = _gen(N2, True)
    host = host_cols(N2, discount=spread(g["discount"], 1, base), quantity=spread(g["quantity"], 2, base))
    cols = upload(gdk, host)
    with images(gdk):
        for dlo, dhi, qmax in ((base + 5, base + 7, base + 2400), (base - 1, base + 3, base + 5000),
                               (5, 7, 2400)):
            assert run_q6(gdk, ora, cols, dlo, dhi, qmax) == model_q6(ora, host, dlo, dhi, qmax)
        assert gdk.colimg_info(cols["discount"]) == (1, 1, base)
        assert gdk.colimg_info(cols["quantity"])[:2] == (1, 2)
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4)


def test_predicate_bounds(gdk, ora):
    """Bounds below, at and above the columns' minimum and maximum, a
    reversed pair, and the ends of the lng range."""
    host = host_cols(N2)
    cols = upload(gdk, host)
    dmin, dmax, qmin, qmax_ = 0, 10, 100, 5000    # the generator's ranges
    for k, lo, hi in (("discount", dmin, dmax), ("quantity", qmin, qmax_)):
        live = host[k][host[k] != NIL64]
        assert (live.min(), live.max()) == (lo, hi)
    assert model_q6(ora, host) == ora_q6(ora, host, 4)
    cases = [(5, 7, 2400)]
    cases += [(lo, hi, 2400) for lo in (dmin - 1, dmin, dmin + 1, dmax, dmax + 1, NIL64, NIL64 + 1)
              for hi in (dmin - 1, dmin, dmax - 1, dmax, dmax + 1, I64MAX)]
    cases += [(7, 5, 2400), (I64MAX, NIL64 + 1, 2400)]
    cases += [(5, 7, q) for q in (qmin - 1, qmin, qmin + 1, qmax_, qmax_ + 1, qmax_ + 2, NIL64 + 1, I64MAX, 0)]
    want = {c: model_q6(ora, host, *c) for c in cases}
    with images(gdk):
        for c in cases:
            assert run_q6(gdk, ora, cols, *c) == want[c], c
        assert gdk.colimg_info(cols["discount"]) == (1, 1, 0)
        assert gdk.colimg_info(cols["quantity"]) == (1, 2, 100)
    # the raw cascade agrees on the same bounds (the translation changes nothing)
    try:
        gdk.q6_set_variant(19, 1)
        for c in cases[::5]:
            assert run_q6(gdk, ora, cols, *c) == want[c], c
    finally:
        gdk.q6_set_variant(IMG, 64)


@pytest.mark.parametrize("which", ["discount", "quantity"])
def test_column_of_nils(gdk, ora, which):
    host = host_cols(N2, **{which: np.full(N2, NIL64, np.int64)})
    cols = upload(gdk, host)
    with images(gdk):
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4) == 0
        assert gdk.colimg_info(cols[which]) == (-1, None, None)


@pytest.mark.parametrize("case", ["none", "price_huge", "price_neg_nil"])
def test_price_ranges(gdk, ora, case):
    """test_q6_value_ranges' prices (+-2^60, negative, nil) through the images."""
    n = 400_009
    host = {k: v.copy() for k, v in ora.tpch_lineitem(13, 0, n, 20_000).items()}
    if case == "price_huge":
        host["extendedprice"][::61] = (1 << 60) + 7
        host["extendedprice"][1::67] = -(1 << 60) - 3
    elif case == "price_neg_nil":
        host["extendedprice"][::13] *= -1
        host["extendedprice"][5::29] = NIL64
    cols = upload(gdk, host)
    with images(gdk):
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4)
        assert gdk.colimg_info(cols["discount"])[:2] == (1, 1)
        assert gdk.colimg_info(cols["quantity"])[:2] == (1, 2)


def test_write_invalidates(gdk, ora):
    """A write through the ABI drops the image; the next Q6 sees the new
    values and the column gets a new image or the ineligible mark."""
    host = host_cols(N2)
    cols = upload(gdk, host)
    with images(gdk):
        first = run_q6(gdk, ora, cols)
        assert first == ora_q6(ora, host, 4)
        assert gdk.colimg_info(cols["discount"]) == (1, 1, 0)
        # BATupload: discounts moved up by two, so other rows qualify
        d2 = spread(host["discount"], 1, 2)
        gdk._chk(gdk.lib().mgdk_BATupload(cols["discount"].ptr, d2.ctypes.data, N2))
        assert gdk.colimg_info(cols["discount"]) == (0, None, None)
        host["discount"] = d2
        second = run_q6(gdk, ora, cols)
        assert second == ora_q6(ora, host, 4) and second != first
        assert gdk.colimg_info(cols["discount"]) == (1, 1, 2)
        # BATappend to all four columns: rows from another part of the table,
        # one of them with a discount far outside
        m = 1000
        extra = {k: host[k][5000:5000 + m].copy() for k in COLS}
        extra["discount"][7] = 1_000_000
        for k in COLS:
            gdk.BATappend(cols[k], gdk.BAT.from_numpy(gdk.TYPE_int if k == "shipdate" else gdk.TYPE_lng, extra[k]))
            host[k] = np.concatenate([host[k], extra[k]])
        assert gdk.colimg_info(cols["discount"]) == (0, None, None)
        assert gdk.colimg_info(cols["quantity"]) == (0, None, None)
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4)
        assert gdk.colimg_info(cols["discount"]) == (-1, None, None)
        assert gdk.colimg_info(cols["quantity"]) == (1, 2, 100)


def test_edited_descriptor(gdk, ora):
    """The descriptor is a public struct: with `count` shrunk by hand on all
    four columns the images built for the longer columns are not used."""
    host = host_cols(N2)
    cols = upload(gdk, host)
    with images(gdk):
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4)
        m = N2 - 70_001
        for k in COLS:
            cols[k].s.count = m
        assert gdk.colimg_info(cols["discount"]) == (0, None, None)
        cut = {k: host[k][:m] for k in COLS}
        assert run_q6(gdk, ora, cols) == ora_q6(ora, cut, 4)
        assert gdk.colimg_info(cols["discount"]) == (1, 1, 0)


def test_slice_views(gdk, ora):
    """BATslice views take no image and give the oracle's answer on the slice."""
    host = host_cols(N2)
    cols = upload(gdk, host)
    with images(gdk):
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4)
        for lo, hi in ((1024, N2 - 5), (3, 300_000)):
            views = {k: gdk.BATslice(cols[k], lo, hi) for k in COLS}
            cut = {k: host[k][lo:hi] for k in COLS}
            assert run_q6(gdk, ora, views) == ora_q6(ora, cut, 4)
            for k in COLS:
                assert gdk.colimg_info(views[k]) == (0, None, None)


def test_images_off(gdk, ora):
    """set_colimg_min(None): no image appears and the launch is the raw cascade's."""
    host = host_cols(N2)
    cols = upload(gdk, host)
    want = ora_q6(ora, host, 4)
    with images(gdk, min_rows=None):
        assert run_q6(gdk, ora, cols) == want
        lines = gdk.q6_last_lines()
        for k in COLS:
            assert gdk.colimg_info(cols[k]) == (0, None, None)
    with images(gdk, min_rows=N2 + 1):     # too small for the policy
        assert run_q6(gdk, ora, cols) == want
        assert gdk.colimg_info(cols["discount"]) == (0, None, None)
    try:
        gdk.q6_set_variant(19, 1)
        assert run_q6(gdk, ora, cols) == want
        assert gdk.q6_last_lines() == lines
    finally:
        gdk.q6_set_variant(IMG, 64)


def _blocks_with_any(mask, rows):
    k = mask.size // rows
    return int(mask[:k * rows].reshape(k, rows).any(axis=1).sum())


def test_line_count(gdk, ora):
    """q6_last_lines of the image variant = the 128-B lines of each array that
    hold a row which passed the earlier predicates: 128 rows per line of the
    1-byte discount image, 64 of the 2-byte quantity image, 16 of
    extendedprice.  The image variants run the cascade on the left-over
    chunks too, so the model covers every full 256-row chunk; the 77 tail
    rows are not counted.  Fewer lines than the raw cascade on the same data."""
    host = host_cols(N2, nils=False)
    cols = upload(gdk, host)
    d0, d1 = ora.mkdate(1994, 1, 1), ora.mkdate(1995, 1, 1)
    full = N2 // 256 * 256
    m1 = ((host["shipdate"] >= d0) & (host["shipdate"] < d1))[:full]
    m2 = m1 & ((host["discount"] >= 5) & (host["discount"] <= 7))[:full]
    m3 = m2 & (host["quantity"] < 2400)[:full]
    want = _blocks_with_any(m1, 128) + _blocks_with_any(m2, 64) + _blocks_with_any(m3, 16)
    with images(gdk):
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4)
        assert gdk.colimg_info(cols["discount"]) == (1, 1, 0)
        assert gdk.colimg_info(cols["quantity"]) == (1, 2, 100)
        got = gdk.q6_last_lines()
    print("image lines", got, "model", want)
    assert got == want
    try:
        gdk.q6_set_variant(19, 1)
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4)
        raw = gdk.q6_last_lines()
    finally:
        gdk.q6_set_variant(IMG, 64)
    print("raw cascade lines", raw)
    assert got < raw


def _size_class(nbytes):
    c = 256
    while c < nbytes:
        c *= 2
    return c


def test_concurrent_first_use(gdk, ora):
    """Four threads run Q6 at once on the same fresh columns: all get the
    oracle's revenue and one image per column is built -- device memory grows
    by the two images (1 MiB and 2 MiB blocks here) and the threads' small
    buffers, not by a duplicate image."""
    host = host_cols(N2)
    want = ora_q6(ora, host, 4)
    with images(gdk):
        warm = upload(gdk, host_cols(257))
        run_q6(gdk, ora, warm)
        cols = upload(gdk, host)
        before = int(gdk.lib().mgdk_mem_cursize())
        got, errors = [], []
        gate = threading.Barrier(4)

        def work():
            try:
                gate.wait()
                got.append(run_q6(gdk, ora, cols))
            except Exception as ex:  # noqa: BLE001
                errors.append(repr(ex))

        ts = [threading.Thread(target=work) for _ in range(4)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        after = int(gdk.lib().mgdk_mem_cursize())
        assert not errors, errors
        assert got == [want] * 4
        assert gdk.colimg_info(cols["discount"]) == (1, 1, 0)
        assert gdk.colimg_info(cols["quantity"]) == (1, 2, 100)
    imgs = _size_class(N2) + _size_class(2 * N2)
    assert imgs <= after - before < imgs + (512 << 10), (before, after, imgs)


@pytest.mark.parametrize("variant,n", [(19, N2), (20, N4), (IMG, N2), (IMG4, N4)])
def test_all_loop_regions(gdk, ora, variant, n):
    """The unrolled loop, the left-over loop and the tail rows of the raw
    cascade (19 / 20) and of the image variants, one workgroup per CU."""
    host = host_cols(n)
    cols = upload(gdk, host)
    with images(gdk, variant):
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4)
        assert gdk.q6_last_lines() > 0


@pytest.mark.parametrize("right", [True, False])
def test_known_extremes(gdk, ora, right):
    """A tnonil column whose tminpos / tmaxpos are known is encoded without the
    min/max pass; positions that do not hold the extremes (the descriptor is
    the caller's to edit) are found out by the encode pass and the column is
    scanned after all."""
    host = host_cols(N2, nils=False)
    cols = upload(gdk, host)
    for k in ("discount", "quantity"):
        v, s = host[k], cols[k].s
        assert s.tnonil == 1
        s.tminpos = int(np.argmin(v)) if right else int(np.flatnonzero(v != v.min())[0])
        s.tmaxpos = int(np.argmax(v)) if right else int(np.flatnonzero(v != v.max())[-1])
    with images(gdk):
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4)
        assert gdk.colimg_info(cols["discount"]) == (1, 1, 0)
        assert gdk.colimg_info(cols["quantity"]) == (1, 2, 100)
