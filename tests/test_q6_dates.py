"""The fused Q6 reading shipdate through a column image too (DESIGN.md §3,
§4): the wide variants (26 / 27) of k_q6s, 512-row chunks with 8 rows per
lane.  Every revenue is compared with `==`: with the oracle's ora.q6 at the
query's standard bounds, and with an exact integer restatement of the raw
predicate for other bounds, which is itself checked against ora.q6 at the
standard bounds.

Sizes: at q6_set_variant(v, 1) the grid is 256 workgroups = 1024 waves of
one CH = 512-row chunk each, so n = CH * (U * 1024 + 512) + 77 rows runs the
loop over U chunks at a time once on every wave, one more chunk on the first
512 waves (for variant 26 a chunk whose shipdates were prefetched, while the
other waves find no next chunk; for variant 27 its left-over loop) and 77
tail rows.  U = 1 for variant 26, U = 2 for variant 27.
"""
import functools
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest

gpu = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CH = 512
WIDE, WIDE2 = 26, 27                 # one chunk at a time with prefetch / 2 chunks in flight
UNROLL = {WIDE: 1, WIDE2: 2}
NIL32, NIL64 = np.iinfo(np.int32).min, np.iinfo(np.int64).min
I32MAX = np.iinfo(np.int32).max
COLS = ("shipdate", "discount", "quantity", "extendedprice")


def rows_for(variant):
    return CH * (UNROLL[variant] * 1024 + 512) + 77


N1, N2 = rows_for(WIDE), rows_for(WIDE2)     # 786,509 and 1,310,797


@functools.lru_cache(maxsize=None)
def _gen(n, nils):
    """Generator columns (shared, read-only), with 1 % nils in all four."""
    from oracle import pyoracle as ora
    host = ora.tpch_lineitem(17, 0, n, 20_000)
    host = {k: host[k] for k in COLS}
    if nils:
        r = np.random.default_rng(67)
        for k in COLS:
            host[k][r.random(n) < 0.01] = NIL32 if k == "shipdate" else NIL64
    for v in host.values():
        v.setflags(write=False)
    return host


def host_cols(n, nils=True, **changed):
    h = dict(_gen(n, nils))
    h.update(changed)
    return h


def upload(gdk, host, date_type=None):
    tp = {k: gdk.TYPE_lng for k in COLS}
    tp["shipdate"] = gdk.TYPE_int if date_type is None else date_type
    return {k: gdk.BAT.from_numpy(tp[k], host[k]) for k in COLS}


def std_dates(ora):
    return ora.mkdate(1994, 1, 1), ora.mkdate(1995, 1, 1)


def run_q6(gdk, ora, cols, d0=None, d1=None, dlo=5, dhi=7, qmax=2400):
    s0, s1 = std_dates(ora)
    return gdk.q6_fused(cols["shipdate"], cols["discount"], cols["quantity"], cols["extendedprice"],
                        s0 if d0 is None else d0, s1 if d1 is None else d1, dlo, dhi, qmax)


def ora_q6(ora, host, threads=4):
    n = host["shipdate"].shape[0]
    li = {k: np.ascontiguousarray(host[k]) for k in COLS}
    li["tax"] = np.zeros(n, np.int64)
    li["returnflag"] = np.zeros(n, np.uint8)
    li["linestatus"] = np.zeros(n, np.uint8)
    return ora.q6(li, threads)


def model_q6(ora, host, d0=None, d1=None, dlo=5, dhi=7, qmax=2400):
    """The raw predicate and the exact sum of products.  The products are
    summed in int64 where the columns' magnitudes show that no partial sum
    can leave it, else in Python integers."""
    s0, s1 = std_dates(ora)
    d0 = s0 if d0 is None else d0
    d1 = s1 if d1 is None else d1
    sd, di, q, p = (host[k] for k in COLS)
    ok = (sd != NIL32) & (sd >= d0) & (sd < d1) & (di != NIL64) & (q != NIL64) & (p != NIL64)
    ok &= (di >= dlo) & (di <= dhi) & (q < qmax)
    ps, ds = p[ok], di[ok]
    if ps.size == 0:
        return 0
    if int(np.abs(ps).max()) * int(np.abs(ds).max()) * ps.size < (1 << 62):
        return int(np.dot(ps, ds))
    return sum(int(a) * int(b) for a, b in zip(ps, ds))


class wide:
    """A wide variant at `bpc` workgroups per CU, images from `min_rows` up."""

    def __init__(self, gdk, variant=WIDE, bpc=1, min_rows=1):
        self.gdk, self.variant, self.bpc, self.min_rows = gdk, variant, bpc, min_rows

    def __enter__(self):
        self.prev = self.gdk.set_colimg_min(self.min_rows)
        self.gdk.q6_set_variant(self.variant, self.bpc)

    def __exit__(self, *exc):
        self.gdk.q6_set_variant(WIDE, 64)
        self.gdk.set_colimg_min(self.prev)


def spread(col, kind, nil=NIL64, far=40_000):
    """col given the spread of an image of width 2 (one outlier within
    65534 of the rest), of none (kind 0: outliers further apart than that),
    or left as it is (kind 1 for the generator's discount)."""
    out = col.copy()
    live = out != nil
    first = np.flatnonzero(live)[:2]
    if kind == 2:
        out[first[0]] = out[live].min() - far
    elif kind == 0:
        out[first[0]] = out[live].min() - far
        out[first[1]] = out[live].max() + far
    return out


def narrow_qty(q):
    """quantity squeezed into 2300 .. 2496 (a 1-byte image; about half of it
    below the query's 2400)"""
    out = q.copy()
    live = out != NIL64
    out[live] = 2300 + (out[live] - 100) // 25
    return out


def ship(sd, kind, d0):
    """shipdate with the spread of a 2-byte image (as generated: about
    2,700 codes), of a 1-byte image (200 codes straddling d0), or of none
    (one date more than 65534 codes below the rest)."""
    out = sd.copy()
    live = out != NIL32
    if kind == 1:
        out[live] = d0 - 100 + (out[live] - out[live].min()) % 200
    elif kind == 0:
        out[np.flatnonzero(live)[0]] = out[live].min() - 70_000
    return out


def info_want(col, w, nil):
    live = col[col != nil]
    return (1, w, int(live.min())) if w else (-1, None, None)


@gpu
@pytest.mark.parametrize("sw", [2, 1, 0])
@pytest.mark.parametrize("dw", [1, 2, 0])
@pytest.mark.parametrize("qw", [2, 1, 0])
def test_width_combinations(gdk, ora, sw, dw, qw):
    """All 27 combinations of image widths (0: no image, the column is read
    raw by the same kernel) on data with nils in all four columns, and the
    states colimg_info reports."""
    g = _gen(N1, True)
    host = host_cols(N1, shipdate=ship(g["shipdate"], sw, std_dates(ora)[0]),
                     discount=spread(g["discount"], dw),
                     quantity=narrow_qty(g["quantity"]) if qw == 1 else spread(g["quantity"], qw))
    cols = upload(gdk, host)
    with wide(gdk):
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4)
        assert gdk.colimg_info(cols["shipdate"]) == info_want(host["shipdate"], sw, NIL32)
        assert gdk.colimg_info(cols["discount"]) == info_want(host["discount"], dw, NIL64)
        assert gdk.colimg_info(cols["quantity"]) == info_want(host["quantity"], qw, NIL64)
        assert gdk.colimg_info(cols["extendedprice"]) == (0, None, None)
        assert gdk.q6_last_lines() > 0


@gpu
@pytest.mark.parametrize("sw,dw,qw", [(2, 1, 2), (1, 0, 1), (0, 2, 0), (2, 0, 0), (0, 1, 2)])
def test_two_chunks_in_flight(gdk, ora, sw, dw, qw):
    """Variant 27: the loop over two chunks, its left-over loop and the tail."""
    g = _gen(N2, True)
    host = host_cols(N2, shipdate=ship(g["shipdate"], sw, std_dates(ora)[0]),
                     discount=spread(g["discount"], dw),
                     quantity=narrow_qty(g["quantity"]) if qw == 1 else spread(g["quantity"], qw))
    cols = upload(gdk, host)
    with wide(gdk, WIDE2):
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4)
        assert gdk.colimg_info(cols["shipdate"]) == info_want(host["shipdate"], sw, NIL32)


def date_cases(smin, smax, d0s, d1s):
    edge = [smin - 1, smin, smin + 1, smax - 1, smax, smax + 1, NIL32, NIL32 + 1, I32MAX]
    cases = [(a, b) for a in edge for b in edge]             # holds d0 == d1 and d0 > d1
    mid = (smin + smax) // 2
    cases += [(d0s, d1s), (d1s, d0s), (mid, mid), (mid, mid + 1), (mid + 1, mid), (d0s, I32MAX), (NIL32, d1s)]
    return cases


@gpu
@pytest.mark.parametrize("sw", [2, 1, 0])
def test_date_bounds(gdk, ora, sw):
    """d0 and d1 below, at and above the column's minimum and maximum, equal,
    reversed, and at the ends of the int range, against the model -- on a
    2-byte image, a 1-byte image and the raw column."""
    d0s, d1s = std_dates(ora)
    g = _gen(N1, True)
    host = host_cols(N1, shipdate=ship(g["shipdate"], sw, d0s))
    assert model_q6(ora, host) == ora_q6(ora, host, 4)
    live = host["shipdate"][host["shipdate"] != NIL32]
    smin, smax = int(live.min()), int(live.max())
    cases = date_cases(smin, smax, d0s, d1s)
    if sw != 2:
        cases = cases[::3] + cases[-7:]
    want = {c: model_q6(ora, host, *c) for c in cases}
    assert len(set(want.values())) > 3
    cols = upload(gdk, host)
    with wide(gdk):
        for c in cases:
            assert run_q6(gdk, ora, cols, *c) == want[c], c
        assert gdk.colimg_info(cols["shipdate"]) == info_want(host["shipdate"], sw, NIL32)
    if sw == 2:
        # the raw cascade agrees on the same bounds
        try:
            gdk.q6_set_variant(19, 1)
            for c in cases[::7]:
                assert run_q6(gdk, ora, cols, *c) == want[c], c
        finally:
            gdk.q6_set_variant(WIDE, 64)


@gpu
def test_shipdates_all_nil(gdk, ora):
    host = host_cols(N1, shipdate=np.full(N1, NIL32, np.int32))
    cols = upload(gdk, host)
    with wide(gdk):
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4) == 0
        assert run_q6(gdk, ora, cols, NIL32, I32MAX) == 0
        assert gdk.colimg_info(cols["shipdate"]) == (-1, None, None)


@gpu
@pytest.mark.parametrize("n", [1, 7, 8, 9, CH - 1, CH, CH + 1])
def test_small_columns(gdk, ora, n):
    host = {k: v[3000:3000 + n] for k, v in _gen(N1, True).items()}
    cols = upload(gdk, host)
    with wide(gdk):
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 1)
        assert run_q6(gdk, ora, cols, NIL32, I32MAX, 0, 10, 5001) == model_q6(ora, host, NIL32, I32MAX, 0, 10, 5001)
        if (host["shipdate"] != NIL32).any():
            assert gdk.colimg_info(cols["shipdate"])[0] == 1


@gpu
def test_slice_views(gdk, ora):
    """BATslice views take no image and give the oracle's answer on the slice."""
    host = host_cols(N1)
    cols = upload(gdk, host)
    with wide(gdk):
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4)
        for lo, hi in ((1024, N1 - 5), (3, 300_000)):
            views = {k: gdk.BATslice(cols[k], lo, hi) for k in COLS}
            cut = {k: host[k][lo:hi] for k in COLS}
            assert run_q6(gdk, ora, views) == ora_q6(ora, cut, 4)
            for k in COLS:
                assert gdk.colimg_info(views[k]) == (0, None, None)


@gpu
def test_date_typed_shipdate(gdk, ora):
    """A TYPE_date shipdate gets the same image as the TYPE_int one."""
    host = host_cols(N1)
    want = ora_q6(ora, host, 4)
    with wide(gdk):
        for tp in (gdk.TYPE_date, gdk.TYPE_int):
            cols = upload(gdk, host, date_type=tp)
            assert cols["shipdate"].ttype == tp
            assert run_q6(gdk, ora, cols) == want
            assert gdk.colimg_info(cols["shipdate"]) == info_want(host["shipdate"], 2, NIL32)


@gpu
def test_write_invalidates(gdk, ora):
    """BATupload and BATappend to shipdate drop its image; the next call sees
    the new values and rebuilds the image or marks the column ineligible."""
    d0s, _ = std_dates(ora)
    host = host_cols(N1)
    cols = upload(gdk, host)
    with wide(gdk):
        first = run_q6(gdk, ora, cols)
        assert first == ora_q6(ora, host, 4)
        assert gdk.colimg_info(cols["shipdate"]) == info_want(host["shipdate"], 2, NIL32)
        s2 = ship(host["shipdate"], 1, d0s)
        gdk._chk(gdk.lib().mgdk_BATupload(cols["shipdate"].ptr, s2.ctypes.data, N1))
        assert gdk.colimg_info(cols["shipdate"]) == (0, None, None)
        host["shipdate"] = s2
        second = run_q6(gdk, ora, cols)
        assert second == ora_q6(ora, host, 4) and second != first
        assert gdk.colimg_info(cols["shipdate"]) == info_want(s2, 1, NIL32)
        # BATappend to all four columns, one of the new dates far outside
        m = 1000
        extra = {k: _gen(N1, True)[k][5000:5000 + m].copy() for k in COLS}
        extra["shipdate"][7] = d0s + 1_000_000
        for k in COLS:
            gdk.BATappend(cols[k], gdk.BAT.from_numpy(gdk.TYPE_int if k == "shipdate" else gdk.TYPE_lng, extra[k]))
            host[k] = np.concatenate([host[k], extra[k]])
        assert gdk.colimg_info(cols["shipdate"]) == (0, None, None)
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4)
        assert gdk.colimg_info(cols["shipdate"]) == (-1, None, None)
        assert gdk.colimg_info(cols["discount"]) == (1, 1, 0)


def _blocks_with_any(mask, rows):
    k = mask.size // rows
    return int(mask[:k * rows].reshape(k, rows).any(axis=1).sum())


def line_model(ora, host, lo, hi):
    """128-B lines of the 1-byte discount image, the 2-byte quantity image
    and raw extendedprice that hold a row of [lo, hi) which passed the
    earlier predicates (lo, hi multiples of 128)."""
    d0, d1 = std_dates(ora)
    m1 = ((host["shipdate"] >= d0) & (host["shipdate"] < d1))[lo:hi]
    m2 = m1 & ((host["discount"] >= 5) & (host["discount"] <= 7))[lo:hi]
    m3 = m2 & (host["quantity"] < 2400)[lo:hi]
    return _blocks_with_any(m1, 128) + _blocks_with_any(m2, 64) + _blocks_with_any(m3, 16)


@gpu
@pytest.mark.parametrize("extra", [0, 256])
def test_line_and_byte_counts(gdk, ora, extra):
    """On data without nils: q6_last_lines of the wide variant is the model
    over all full 512-row chunks, q6_last_bytes is the rows at the shipdate
    image's 2 bytes plus 128 bytes per line.  Variant 24 runs the cascade
    over all full 256-row chunks: the same rows when n mod 512 < 256 (extra
    0: equal counts), one more 256-row chunk otherwise (extra 256: it counts
    exactly the model's lines of that chunk more)."""
    n = N1 + extra
    host = host_cols(n, nils=False)
    cols = upload(gdk, host)
    full = n // CH * CH
    want = line_model(ora, host, 0, full)
    with wide(gdk):
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4)
        assert gdk.colimg_info(cols["shipdate"])[:2] == (1, 2)
        assert gdk.colimg_info(cols["discount"]) == (1, 1, 0)
        assert gdk.colimg_info(cols["quantity"]) == (1, 2, 100)
        got, nbytes = gdk.q6_last_lines(), gdk.q6_last_bytes()
    print("wide lines", got, "model", want, "bytes", nbytes)
    assert got == want
    assert nbytes == n * 2 + 128 * got
    try:
        gdk.q6_set_variant(24, 1)
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4)
        lines24, bytes24 = gdk.q6_last_lines(), gdk.q6_last_bytes()
    finally:
        gdk.q6_set_variant(WIDE, 64)
    more = line_model(ora, host, full, full + 256) if n - full >= 256 else 0
    print("variant 24 lines", lines24, "of them in the extra 256-row chunk", more)
    assert (more > 0) == (extra == 256)
    assert lines24 == got + more
    assert bytes24 == n * 4 + 128 * lines24


def _size_class(nbytes):
    c = 256
    while c < nbytes:
        c *= 2
    return c


MARGIN = 512 << 10


def test_size_classes_of_three_images():
    """On the CPU: at N1 rows the three images fill the classes 2 MiB, 1 MiB
    and 2 MiB, and the smallest of them is larger than the 512 KiB margin of
    test_concurrent_first_use, so a duplicate of any image would show."""
    classes = [_size_class(2 * N1), _size_class(N1), _size_class(2 * N1)]
    assert classes == [2 << 20, 1 << 20, 2 << 20]
    assert min(classes) > MARGIN
    assert all(c >= need for c, need in zip(classes, (2 * N1, N1, 2 * N1)))


@gpu
def test_concurrent_first_use(gdk, ora):
    """Four threads make first use on fresh columns at once: all get the
    oracle's revenue and one image per column is built -- device memory grows
    by the three images' size classes and the threads' small buffers."""
    host = host_cols(N1)
    want = ora_q6(ora, host, 4)
    with wide(gdk):
        warm = upload(gdk, host_cols(CH + 1))
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
        assert gdk.colimg_info(cols["shipdate"])[:2] == (1, 2)
        assert gdk.colimg_info(cols["discount"]) == (1, 1, 0)
        assert gdk.colimg_info(cols["quantity"]) == (1, 2, 100)
    imgs = _size_class(2 * N1) + _size_class(N1) + _size_class(2 * N1)
    assert imgs <= after - before < imgs + MARGIN, (before, after, imgs)


@gpu
def test_images_off(gdk, ora):
    """set_colimg_min(None): the oracle's revenue and no image; a variant
    below 26 never asks for a shipdate image."""
    host = host_cols(N1)
    cols = upload(gdk, host)
    want = ora_q6(ora, host, 4)
    with wide(gdk, min_rows=None):
        assert run_q6(gdk, ora, cols) == want
        assert gdk.q6_last_bytes() == N1 * 4 + 128 * gdk.q6_last_lines()
        for k in COLS:
            assert gdk.colimg_info(cols[k]) == (0, None, None)
    with wide(gdk, min_rows=N1 + 1):       # too small for the policy
        assert run_q6(gdk, ora, cols) == want
        assert gdk.colimg_info(cols["shipdate"]) == (0, None, None)
    with wide(gdk, 24):
        assert run_q6(gdk, ora, cols) == want
        assert gdk.colimg_info(cols["shipdate"]) == (0, None, None)
        assert gdk.colimg_info(cols["discount"]) == (1, 1, 0)


def test_date_code_range_matches_raw_predicate(tmp_path):
    """tests/q6dates_check.cpp on the CPU, under -fsanitize=undefined where
    the compiler links it."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(HERE, "q6dates_check.cpp")
    exe = str(tmp_path / "q6dates_check")
    base = [cxx, "-std=c++17", "-O1", "-Wall", src, "-o", exe]
    san = ["-fsanitize=undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(base + san, capture_output=True, text=True).returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)   # no sanitizer runtime here
        assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith(" 0 wrong")
