"""The fused Q6 over packed column images (Priv::pimg,
variant 28, q6p::k_q6s): shipdate, discount and quantity read through codes
of 4 / 8 / 12 / 16 bits per row, code = (value - base) / stride.  Every
revenue is compared with `==`: with the oracle's ora.q6 at the query's
standard bounds, and with test_q6_dates.model_q6 -- an exact integer
restatement of the raw predicate, itself checked against ora.q6 -- for other
bounds.

Sizes: at q6_set_variant(28, 1) the grid is 256 workgroups = 1024 waves of
one 512-row chunk each, so n = 512 * (1024 + 512) + 77 = 786,509 rows gives
every wave one chunk, the first 512 waves a second chunk whose codes were
prefetched while the other waves find no next chunk, and 77 tail rows.
"""
import math
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest

from test_q6_dates import (CH, COLS, I32MAX, MARGIN, N1, NIL32, NIL64, _blocks_with_any, _gen, _size_class,
                           host_cols, model_q6, ora_q6, run_q6, std_dates, upload)

gpu = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PACK, WIDE = 28, 26
I64MAX = np.iinfo(np.int64).max
WIDTHS = (4, 8, 12, 16)
N = N1
assert N == 512 * (1024 + 512) + 77


class packed:
    """Variant `variant` at `bpc` workgroups per CU, images from `min_rows` up;
    leaves the default (28 at 64) behind."""

    def __init__(self, gdk, variant=PACK, bpc=1, min_rows=1):
        self.gdk, self.variant, self.bpc, self.min_rows = gdk, variant, bpc, min_rows

    def __enter__(self):
        self.prev = self.gdk.set_colimg_min(self.min_rows)
        self.gdk.q6_set_variant(self.variant, self.bpc)

    def __exit__(self, *exc):
        self.gdk.q6_set_variant(PACK, 64)
        self.gdk.set_colimg_min(self.prev)


def pack_want(col, nil):
    """colpack_info as computed on the host."""
    live = col[col != nil].astype(object)
    if live.size == 0:
        return (-1, None, None, None)
    base = int(live.min())
    stride = int(math.gcd(*set(int(x) - base for x in np.unique(col[col != nil])))) or 1
    maxcode = (int(live.max()) - base) // stride
    for w in WIDTHS:
        if maxcode <= (1 << w) - 2:
            return (1, w, base, stride)
    return (-1, None, None, None)


def _first_live(col, nil, k=1):
    return np.flatnonzero(col != nil)[:k]


def outlier(col, nil, below):
    """one value `below` under the smallest"""
    out = col.copy()
    out[_first_live(out, nil)[0]] = out[out != nil].min() - below
    return out


def ship_w(sd, w, d0):
    """shipdate in the width class w: 15 codes and 200 codes straddling d0,
    the generated 2,700 or so, and one outlier 40,000 below them."""
    out = sd.copy()
    live = out != NIL32
    if w == 4:
        out[live] = d0 - 7 + (out[live] - out[live].min()) % 15
    elif w == 8:
        out[live] = d0 - 100 + (out[live] - out[live].min()) % 200
    elif w == 16:
        out = outlier(out, NIL32, 40_000)
    return out


def disc_w(di, w):
    """discount 0 .. 10 as generated (4 bits), or with one outlier 200 / 3,000 /
    40,000 below"""
    return di if w == 4 else outlier(di, NIL64, {8: 200, 12: 3_000, 16: 40_000}[w])


def qty_w(q, w):
    """quantity as generated (50 codes of stride 100: 8 bits), squeezed into
    15 codes of stride 50 around the query's 2400, or with one outlier 3,000 /
    40,000 strides below"""
    if w == 8:
        return q
    out = q.copy()
    live = out != NIL64
    if w == 4:
        out[live] = 2000 + (out[live] - 100) // 100 % 15 * 50
        return out
    return outlier(out, NIL64, 100 * {12: 3_000, 16: 40_000}[w])


@gpu
@pytest.mark.parametrize("sw", WIDTHS)
@pytest.mark.parametrize("dw", WIDTHS)
@pytest.mark.parametrize("qw", WIDTHS)
def test_width_combinations(gdk, ora, sw, dw, qw):
    """All 64 combinations of packed widths on data with nils in all four
    columns, and colpack_info as computed on the host."""
    g = _gen(N, True)
    host = host_cols(N, shipdate=ship_w(g["shipdate"], sw, std_dates(ora)[0]), discount=disc_w(g["discount"], dw),
                     quantity=qty_w(g["quantity"], qw))
    want = {k: pack_want(host[k], NIL32 if k == "shipdate" else NIL64) for k in COLS[:3]}
    assert [want[k][1] for k in COLS[:3]] == [sw, dw, qw]
    cols = upload(gdk, host)
    with packed(gdk):
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4)
        for k in COLS[:3]:
            assert gdk.colpack_info(cols[k]) == want[k], k
            assert gdk.colimg_info(cols[k]) == (0, None, None)       # the default path builds no byte image
        assert gdk.colpack_info(cols["extendedprice"]) == (0, None, None, None)
        assert gdk.q6_last_lines() > 0
        assert gdk.q6_last_bytes() == N * (sw + dw + qw) // 8 + 128 * gdk.q6_last_lines()


@gpu
def test_strides(gdk, ora):
    g = _gen(N, True)
    q101 = g["quantity"].copy()
    q101[_first_live(q101, NIL64)[0]] = 101
    const = np.where(g["quantity"] != NIL64, 1700, NIL64)
    with packed(gdk):
        cols = upload(gdk, host_cols(N))
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host_cols(N), 4)
        assert gdk.colpack_info(cols["quantity"]) == (1, 8, 100, 100)
        assert gdk.colpack_info(cols["discount"]) == (1, 4, 0, 1)
        for q, info in ((q101, (1, 16, 100, 1)), (const, (1, 4, 1700, 1))):
            host = host_cols(N, quantity=q)
            cols = upload(gdk, host)
            assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4)
            assert gdk.colpack_info(cols["quantity"]) == info


@gpu
def test_discount_off_stride_bounds(gdk, ora):
    """discount x 10 (stride 10): bounds on and off the stride select what the
    raw predicate selects."""
    g = _gen(N, True)
    d10 = np.where(g["discount"] != NIL64, g["discount"] * 10, NIL64)
    host = host_cols(N, discount=d10)
    cases = [(50, 70), (45, 75), (41, 69), (51, 79), (49, 50), (51, 59), (-5, 5), (95, 105), (100, 100), (101, 200),
             (70, 50)]
    want = {c: model_q6(ora, host, dlo=c[0], dhi=c[1]) for c in cases}
    assert len(set(want.values())) > 5 and want[(51, 59)] == 0
    cols = upload(gdk, host)
    with packed(gdk):
        for c in cases:
            assert run_q6(gdk, ora, cols, dlo=c[0], dhi=c[1]) == want[c], c
        assert gdk.colpack_info(cols["discount"]) == (1, 4, 0, 10)


def edges(lo, hi, tmin, tmax):
    return [lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, tmin, tmin + 1, tmax]


@gpu
def test_bounds(gdk, ora):
    """Each bound at the column's smallest and largest value and one either
    side, at the ends of its type, reversed pairs, qmax around 2400 and d1 =
    INT32_MIN, against the model."""
    host = host_cols(N)
    assert model_q6(ora, host) == ora_q6(ora, host, 4)
    d0s, d1s = std_dates(ora)
    live = {k: host[k][host[k] != (NIL32 if k == "shipdate" else NIL64)] for k in COLS[:3]}
    lo = {k: int(v.min()) for k, v in live.items()}
    hi = {k: int(v.max()) for k, v in live.items()}
    se = edges(lo["shipdate"], hi["shipdate"], NIL32, I32MAX)
    de = edges(lo["discount"], hi["discount"], NIL64, I64MAX)
    qe = edges(lo["quantity"], hi["quantity"], NIL64, I64MAX) + [2399, 2400, 2401]
    cases = [dict(d0=a, d1=b) for a in se for b in se]                 # holds equal and reversed pairs
    cases += [dict(d0=d0s, d1=NIL32), dict(d0=d1s, d1=d0s), dict(d0=NIL32, d1=d1s)]
    cases += [dict(dlo=a, dhi=b) for a in de for b in de]
    cases += [dict(qmax=q) for q in qe]
    cases += [dict(d0=NIL32, d1=I32MAX, dlo=NIL64, dhi=I64MAX, qmax=q) for q in qe]
    want = [model_q6(ora, host, **c) for c in cases]
    assert len(set(want)) > 12
    cols = upload(gdk, host)
    with packed(gdk):
        for c, w in zip(cases, want):
            assert run_q6(gdk, ora, cols, **c) == w, c
        assert gdk.colpack_info(cols["shipdate"])[:2] == (1, 12)
    # variant 26 agrees on a sample of the same bounds
    with packed(gdk, WIDE):
        for c, w in list(zip(cases, want))[::9]:
            assert run_q6(gdk, ora, cols, **c) == w, c


OPEN = dict(d0=NIL32 + 1, d1=I32MAX, dlo=NIL64 + 1, dhi=I64MAX, qmax=I64MAX)


@gpu
def test_every_row_passes(gdk, ora):
    """Bounds wide open on data without nils: all 512 rows of every chunk pass,
    every lane runs its loop over 8 set bits."""
    host = host_cols(N, nils=False)
    want = model_q6(ora, host, **OPEN)
    assert want == int(np.dot(host["extendedprice"], host["discount"]))
    cols = upload(gdk, host)
    with packed(gdk):
        assert run_q6(gdk, ora, cols, **OPEN) == want
        assert gdk.q6_last_lines() == N // CH * (CH // 16)


@gpu
def test_one_lane_with_eight_rows(gdk, ora):
    """The only passing rows are the 8 rows of one lane (lane 37 of chunk 700)."""
    d0s, d1s = std_dates(ora)
    g = _gen(N, False)
    sd = np.where(g["shipdate"] >= d0s, d1s, g["shipdate"]).astype(np.int32)     # nothing inside [d0s, d1s)
    r0 = CH * 700 + 8 * 37
    sd[r0:r0 + 8] = d0s
    di, q = g["discount"].copy(), g["quantity"].copy()
    di[r0:r0 + 8] = [5, 6, 7, 5, 6, 7, 5, 6]
    q[r0:r0 + 8] = 100
    host = host_cols(N, nils=False, shipdate=sd, discount=di, quantity=q)
    want = sum(int(p) * int(d) for p, d in zip(host["extendedprice"][r0:r0 + 8], di[r0:r0 + 8]))
    assert want == model_q6(ora, host) == ora_q6(ora, host, 4) != 0
    cols = upload(gdk, host)
    with packed(gdk):
        assert run_q6(gdk, ora, cols) == want
        assert gdk.q6_last_lines() == 1


@gpu
@pytest.mark.parametrize("case", ["huge_prices", "negative_base", "flag_edge_on", "flag_edge_off"])
def test_products(gdk, ora, case):
    """The two forms of the product: prices near +-2^62 (the sum taken in
    Python integers), a discount column with a negative base (the general
    signed 64 x 64 product), and discounts whose largest value is the last
    below 2^31 (the 64 x 32 product at its edge) or the first from 2^31 on."""
    g = _gen(N, True)
    ch = {}
    bounds = {}
    if case == "huge_prices":
        p = g["extendedprice"].copy()
        p[::61] = (1 << 62) - 12345
        p[7::61] = -(1 << 62) + 999
        p[g["extendedprice"] == NIL64] = NIL64
        ch["extendedprice"] = p
    elif case == "negative_base":
        ch["discount"] = np.where(g["discount"] != NIL64, g["discount"] - 3, NIL64)
        bounds = dict(dlo=-2, dhi=4)
    else:
        s = ((1 << 31) - 1) // 10 + (case == "flag_edge_off")
        ch["discount"] = np.where(g["discount"] != NIL64, g["discount"] * s, NIL64)
        assert (int(ch["discount"].max()) < 1 << 31) == (case == "flag_edge_on")
        bounds = dict(dlo=5 * s, dhi=10 * s)
    host = host_cols(N, **ch)
    want = model_q6(ora, host, **bounds)
    if not bounds:
        assert want == ora_q6(ora, host, 4)
    assert want != 0
    cols = upload(gdk, host)
    with packed(gdk):
        assert run_q6(gdk, ora, cols, **bounds) == want
        assert gdk.colpack_info(cols["discount"]) == pack_want(host["discount"], NIL64)
        assert gdk.colpack_info(cols["discount"])[1] == 4


@gpu
@pytest.mark.parametrize("which", ["shipdate", "discount", "quantity"])
def test_fallback(gdk, ora, which):
    """One predicate column whose codes do not fit 16 bits: it is marked
    ineligible and the call is variant 26's -- the same lines, byte images
    included."""
    nil = NIL32 if which == "shipdate" else NIL64
    host = host_cols(N, **{which: outlier(_gen(N, True)[which], nil, 70_001)})
    assert pack_want(host[which], nil) == (-1, None, None, None)
    want = ora_q6(ora, host, 4)
    cols = upload(gdk, host)
    with packed(gdk):
        assert run_q6(gdk, ora, cols) == want
        assert gdk.colpack_info(cols[which]) == (-1, None, None, None)
        lines, nbytes = gdk.q6_last_lines(), gdk.q6_last_bytes()
        for k in COLS[:3]:
            assert gdk.colimg_info(cols[k])[0] == (-1 if k == which else 1)
    cols26 = upload(gdk, host)
    with packed(gdk, WIDE):
        assert run_q6(gdk, ora, cols26) == want
        assert (gdk.q6_last_lines(), gdk.q6_last_bytes()) == (lines, nbytes)
        for k in COLS[:3]:
            assert gdk.colpack_info(cols26[k]) == (0, None, None, None)      # variants up to 27 never ask


@gpu
def test_line_and_byte_counts(gdk, ora):
    """On data without nils: q6_last_lines is the 128-B lines of
    extendedprice (16 rows each) that hold a passing row in the full chunks,
    q6_last_bytes the rows at 12 + 4 + 8 bits plus 128 bytes per line."""
    host = host_cols(N, nils=False)
    d0, d1 = std_dates(ora)
    ok = ((host["shipdate"] >= d0) & (host["shipdate"] < d1) & (host["discount"] >= 5) & (host["discount"] <= 7) &
          (host["quantity"] < 2400))
    want = _blocks_with_any(ok[:N // CH * CH], 16)
    cols = upload(gdk, host)
    with packed(gdk):
        assert run_q6(gdk, ora, cols) == ora_q6(ora, host, 4)
        got, nbytes = gdk.q6_last_lines(), gdk.q6_last_bytes()
        assert [gdk.colpack_info(cols[k])[1] for k in COLS[:3]] == [12, 4, 8]
    print("packed lines", got, "model", want, "bytes", nbytes)
    assert got == want
    assert nbytes == N * (12 + 4 + 8) // 8 + 128 * got


@gpu
def test_write_invalidates_and_views(gdk, ora):
    """BATupload to a tail drops its packed image, which the next call rebuilds
    from the new values; a BATslice view gets none."""
    d0s, _ = std_dates(ora)
    host = host_cols(N)
    cols = upload(gdk, host)
    with packed(gdk):
        first = run_q6(gdk, ora, cols)
        assert first == ora_q6(ora, host, 4)
        assert gdk.colpack_info(cols["shipdate"]) == pack_want(host["shipdate"], NIL32)
        s2 = ship_w(host["shipdate"], 8, d0s)
        gdk._chk(gdk.lib().mgdk_BATupload(cols["shipdate"].ptr, s2.ctypes.data, N))
        assert gdk.colpack_info(cols["shipdate"]) == (0, None, None, None)
        host["shipdate"] = s2
        second = run_q6(gdk, ora, cols)
        assert second == ora_q6(ora, host, 4) and second != first
        assert gdk.colpack_info(cols["shipdate"]) == pack_want(s2, NIL32)
        lo, hi = 1024, N - 5
        views = {k: gdk.BATslice(cols[k], lo, hi) for k in COLS}
        assert run_q6(gdk, ora, views) == ora_q6(ora, {k: host[k][lo:hi] for k in COLS}, 4)
        for k in COLS:
            assert gdk.colpack_info(views[k]) == (0, None, None, None)


@gpu
def test_images_off(gdk, ora):
    """set_colimg_min(None) and a threshold above the row count: the oracle's
    revenue and no packed image."""
    host = host_cols(N)
    cols = upload(gdk, host)
    want = ora_q6(ora, host, 4)
    for min_rows in (None, N + 1):
        with packed(gdk, min_rows=min_rows):
            assert run_q6(gdk, ora, cols) == want
            for k in COLS:
                assert gdk.colpack_info(cols[k]) == (0, None, None, None)
                assert gdk.colimg_info(cols[k]) == (0, None, None)


def _pack_bytes(n, wbits):
    return (n + CH - 1) // CH * (CH // 8) * wbits


def test_size_classes_of_three_packed_images():
    """On the CPU: at N rows the three packed images (12, 4 and 8 bits) fill the
    classes 2 MiB, 512 KiB and 1 MiB.  None is smaller than the 512 KiB margin
    of test_concurrent_first_use, which demands a growth strictly below the
    classes plus that margin: a duplicate of any image would show."""
    need = [_pack_bytes(N, w) for w in (12, 4, 8)]
    classes = [_size_class(b) for b in need]
    assert classes == [2 << 20, 512 << 10, 1 << 20]
    assert min(classes) >= MARGIN
    assert all(c >= b for c, b in zip(classes, need))


@gpu
def test_concurrent_first_use(gdk, ora):
    """Four threads make first use on fresh columns at once: all get the
    oracle's revenue and one packed image per column is built -- device memory
    grows by the three images' size classes and the threads' small buffers."""
    host = host_cols(N)
    want = ora_q6(ora, host, 4)
    with packed(gdk):
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
        assert gdk.colpack_info(cols["shipdate"])[:2] == (1, 12)
        assert gdk.colpack_info(cols["discount"]) == (1, 4, 0, 1)
        assert gdk.colpack_info(cols["quantity"]) == (1, 8, 100, 100)
    imgs = sum(_size_class(_pack_bytes(N, w)) for w in (12, 4, 8))
    assert imgs <= after - before < imgs + MARGIN, (before, after, imgs)


def test_packed_code_bounds_and_layout(tmp_path):
    """tests/q6pack_check.cpp on the CPU, under -fsanitize=undefined where
    the compiler links it."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(HERE, "q6pack_check.cpp")
    exe = str(tmp_path / "q6pack_check")
    base = [cxx, "-std=c++17", "-O1", "-Wall", src, "-o", exe]
    san = ["-fsanitize=undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(base + san, capture_output=True, text=True).returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)   # no sanitizer runtime here
        assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith(" 0 wrong")
