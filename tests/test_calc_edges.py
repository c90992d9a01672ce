"""Integer BATcalc add / sub / mul / div / mod at the edges of their types.

The reference here is a model in plain Python integers, which are exact: no C
restatement and no numpy arithmetic on values.  The CPU tests hold the oracle
to the model over all 125 type triples; the GPU tests hold every kernel form
of calc.hip (k_calc_d<OP, CHECK, CA, CB, WA, WB>, the slow k_calc) and the
integer part of k_divmod to it: results at exactly +-max(tp), every overflow
kind (max + 1, the nil pattern -max - 1, each way a 128-bit product leaves its
range), the first-overflow report across waves, workgroups and the second grid
sweep, sub-word loads at every byte offset of a 16-byte word, and two
different candidate lists.

Every value sweep calls the device outside any try: an error there fails the
test.  Every error case names the pair it expects and compares the whole
message."""
import functools
from collections import namedtuple

import numpy as np
import pytest

TYPES = ["bte", "sht", "int", "lng", "hge"]
BITS = {"bte": 8, "sht": 16, "int": 32, "lng": 64, "hge": 128}
RANK = {t: i for i, t in enumerate(TYPES)}
NPT = {"bte": np.int8, "sht": np.int16, "int": np.int32, "lng": np.int64}
OPS = ["+", "-", "*"]
M64 = (1 << 64) - 1
PAIRS = [(a, b) for a in TYPES for b in TYPES]


def tmax(t):
    return (1 << (BITS[t] - 1)) - 1


def tnil(t):
    return -(1 << (BITS[t] - 1))


# ---- the model ------------------------------------------------------------------

class ModelError(Exception):
    """what the reference reports; .pos is the failing candidate"""

    def __init__(self, msg, pos=None):
        super().__init__(msg)
        self.pos = pos


Result = namedtuple("Result", "values count tnil tnonil hseqbase")


def sig_bits(v):
    """significant bits of |v|: the width of its odd part"""
    v = abs(v)
    return (v >> ((v & -v).bit_length() - 1)).bit_length() if v else 0


def long_double(v):
    """v rounded to a 64-bit mantissa, to nearest and ties to even, as the
    conversion of a 128-bit integer to the x87 long double does"""
    a = abs(v)
    sh = a.bit_length() - 64
    if sh <= 0:
        return v
    q, rem, half = a >> sh, a & ((1 << sh) - 1), 1 << (sh - 1)
    if rem > half or (rem == half and q & 1):
        q += 1
    return (q << sh) * (1 if v >= 0 else -1)


def fmt_operand(t, v):
    """%d / %lld, and for hge "%.40Lg (approx. value)" of a long double: 40
    digits hold any 128-bit value, so the text is the rounded value's digits
    (the value's own when it has at most 64 significant bits)"""
    if t == "hge":
        return "%d (approx. value)" % long_double(v)
    return "%d" % v


def exact(op, x, y):
    return x + y if op == "+" else x - y if op == "-" else x * y


def model_calc(op, xs, ys, t1, t2, tp, hseqbase=0):
    """xs / ys: the operand values in candidate order (a constant repeated)"""
    nx, ny, nz, mx = tnil(t1), tnil(t2), tnil(tp), tmax(tp)
    out, nils = [], 0
    for i, (x, y) in enumerate(zip(xs, ys)):
        if x == nx or y == ny:
            out.append(nz)
            nils += 1
            continue
        r = exact(op, x, y)
        if abs(r) > mx:   # -max - 1, the nil pattern, included
            raise ModelError("22003!overflow in calculation %s%s%s." % (fmt_operand(t1, x), op, fmt_operand(t2, y)), i)
        out.append(r)
    return Result(out, len(out), nils != 0, nils == 0, hseqbase)


def wrap(t, v):
    b = BITS[t]
    v &= (1 << b) - 1
    return v - (1 << b) if v >> (b - 1) else v


def divmod_supported(op, t1, t2, tp):
    if op == "/":
        return RANK[tp] >= RANK[t1]
    return RANK[tp] >= min(RANK[t1], RANK[t2])


def model_divmod(op, xs, ys, t1, t2, tp, hseqbase=0):
    """C's / and %: the quotient truncates toward zero; the remainder is
    ((tp) lft) % rgt with the sign of the wrapped dividend"""
    if not divmod_supported(op, t1, t2, tp):
        raise ModelError("not supported")
    nx, ny, nz = tnil(t1), tnil(t2), tnil(tp)
    out, nils = [], 0
    for i, (x, y) in enumerate(zip(xs, ys)):
        if x == nx or y == ny:
            out.append(nz)
            nils += 1
            continue
        if y == 0:
            raise ModelError("22012!division by zero.", i)
        if op == "/":
            q = abs(x) // abs(y)
            out.append(q if (x < 0) == (y < 0) else -q)
        else:
            l = wrap(tp, x)
            m = abs(l) % abs(y)
            out.append(m if l >= 0 else -m)
    return Result(out, len(out), nils != 0, nils == 0, hseqbase)


# ---- the edge generator -----------------------------------------------------------

@functools.lru_cache(None)
def edge_values(t):
    b, m = BITS[t], tmax(t)
    h = 1 << (b // 2)
    pos = [1, 2, 3, 5, 7, m, m - 1, m - 2, h, h + 1, h - 1, 1 << (b - 2)]
    for tp in TYPES:
        if BITS[tp] > b:
            continue
        mp = tmax(tp)
        for k in range(3):
            pos += [mp - k, mp + 1 + k, (mp - k) // 3, (mp - k) // 5, (mp - k) // 7]
        pos += [(mp + 1) // 2, (mp + 1) // 2 - 1]
    if t == "hge":
        pos += [1 << 63, (1 << 63) - 1, 1 << 64, (1 << 64) + 1, (1 << 64) - 1, 1 << 96, 3 << 62, (1 << 126) - 1]
    s = {0}
    for p in pos:
        if 0 < p <= m:
            s.update((p, -p))
    return tuple(sorted(s))


@functools.lru_cache(None)
def split_pairs(op, t1, t2, tp, cap):
    """(fitting xs, fitting ys, overflowing pairs) of the cross product of the
    two edge sets.  The fitting column is thinned to about `cap` rows; pairs
    whose result is within 2 of +-max(tp), pairs of two +-max operands and
    the three nil rows always stay."""
    mx = tmax(tp)
    m1, m2 = tmax(t1), tmax(t2)
    keep, rest, ovf = [], [], []
    for x in edge_values(t1):
        for y in edge_values(t2):
            r = abs(exact(op, x, y))
            if r > mx:
                ovf.append((x, y))
            elif r >= mx - 2 or (abs(x) == m1 and abs(y) == m2):
                keep.append((x, y))
            else:
                rest.append((x, y))
    step = max(1, -(-len(rest) // cap))
    fit = sorted(keep + rest[::step])
    fit.insert(len(fit) // 3, (tnil(t1), 3))
    fit.insert(2 * len(fit) // 3, (5, tnil(t2)))
    fit.append((tnil(t1), tnil(t2)))
    return tuple(p[0] for p in fit), tuple(p[1] for p in fit), tuple(ovf)


def assert_reaches_both_ends(op, t1, t2, tp, fx, fy, ovf):
    """where anything can overflow, the fitting column holds +max and -max"""
    if not ovf:
        return
    n1, n2 = tnil(t1), tnil(t2)
    rs = {exact(op, x, y) for x, y in zip(fx, fy) if x != n1 and y != n2}
    assert tmax(tp) in rs and -tmax(tp) in rs, (op, t1, t2, tp)


def printable(t, v):
    return t != "hge" or sig_bits(v) <= 64


def msg_pairs(t1, t2, pairs):
    """The pairs whose message the model can print from the value's own
    digits: every hge operand has at most 64 significant bits.  Only where no
    such pair exists the rounded text (long_double) is relied on."""
    good = [p for p in pairs if printable(t1, p[0]) and printable(t2, p[1])]
    for x, y in good:
        assert (t1 != "hge" or sig_bits(x) <= 64) and (t2 != "hge" or sig_bits(y) <= 64)
    return good or list(pairs)


def pool(t):
    """edge values and +-2^k: where pairs with one exact result are looked for"""
    s = set(edge_values(t))
    for k in range(BITS[t] - 1):
        s.update((1 << k, -(1 << k)))
    if t == "hge":
        for m in (3, 5, 7, 15, M64):
            for k in range(0, 128, 3):
                if m << k <= tmax(t):
                    s.update((m << k, -(m << k)))
    return sorted(s, key=lambda v: (abs(v), v))


@functools.lru_cache(None)
def pairs_with_result(op, t1, t2, target):
    """operand pairs from the pools with exact result == target"""
    p2 = set(pool(t2))
    out = []
    for x in pool(t1):
        if op == "+":
            y = target - x
        elif op == "-":
            y = x - target
        else:
            if x == 0 or target % x:
                continue
            y = target // x
        if y in p2 and y != tnil(t2):
            out.append((x, y))
    return tuple(msg_pairs(t1, t2, out))


def mul_exit(x, y):
    """which way the product of two 128-bit values leaves 128 bits (the four
    exits of a schoolbook 64 x 64 multiply, and the nil pattern), else None"""
    ua, ub = abs(x), abs(y)
    ah, al, bh, bl = ua >> 64, ua & M64, ub >> 64, ub & M64
    if ah and bh:
        return "both_high"
    mid = ah * bl + bh * al
    if mid >> 64:
        return "cross"
    res = al * bl + (mid << 64)
    if res >> 128:
        return "carry"
    if res == 1 << 127:
        return "nil_pattern" if (x < 0) != (y < 0) else "max+1"
    if res >> 127:
        return "top"
    return None


@functools.lru_cache(None)
def hge_kinds(op, t1, t2):
    """{kind: pair} of the ways out of 128 bits for a triple into hge with an
    hge operand; every hge operand printable"""
    out = {}
    if op == "*":
        # a "quiet" pair is preferred: the low 128 bits of the product of the
        # magnitudes are below 2^127, a value in range, so nothing but the
        # exit itself can notice it
        found = {}
        for x in pool(t1):
            if x <= 0 or not printable(t1, x):
                continue
            for y in pool(t2):
                k = mul_exit(x, y)
                if k is None or k == "max+1" or not printable(t2, y):
                    continue
                quiet = k == "top" or (abs(x * y) & ((1 << 128) - 1)) < 1 << 127
                if k not in found or (quiet and not found[k][1]):
                    found[k] = ((x, y), quiet)
        need = {"cross", "top", "nil_pattern"} | ({"both_high", "carry"} if t1 == t2 == "hge" else set())
        assert need <= set(found), (t1, t2, sorted(found))
        assert all(found[k][1] for k in need - {"nil_pattern"}), (t1, t2, found)
        out = {k: v[0] for k, v in found.items()}
        assert exact("*", *out["nil_pattern"]) == -(1 << 127)
    else:
        top = (1 << 127) - (1 << 63)   # 64 significant bits
        sg = 1 if op == "+" else -1
        if t1 == "hge" and t2 == "hge":
            out["wrap_up"] = (top, sg * (1 << 64))
            out["wrap_down"] = (-top, -sg * (1 << 64))
            out["wrap_up_max"] = (tmax("hge"), sg * 1)      # (2^127 - 1) + 1
            out["wrap_down_max"] = (-tmax("hge"), -sg * 2)  # -(2^127 - 1) - 2
        elif t1 == "hge":
            out["wrap_up"] = (tmax("hge"), sg * 3)
            out["wrap_down"] = (-tmax("hge"), -sg * 3)
        else:
            out["wrap_up"] = (3, sg * tmax("hge")) if op == "+" else (3, -tmax("hge") + 1)
            out["wrap_down"] = (-3, -tmax("hge")) if op == "+" else (-3, tmax("hge"))
        for x, y in out.values():
            assert abs(exact(op, x, y)) > tmax("hge")
    return out


def overflow_kinds(op, t1, t2, tp):
    """[(kind, pair)] for (b): max + 1, -max - 1, and for hge the 128-bit exits"""
    mx = tmax(tp)
    kinds = []
    for name, target in (("max+1", mx + 1), ("-max-1", -mx - 1)):
        ps = pairs_with_result(op, t1, t2, target)
        assert ps, (op, t1, t2, tp, name)
        kinds.append((name, ps[0]))
    if tp == "hge" and "hge" in (t1, t2):
        kinds += sorted(hge_kinds(op, t1, t2).items())
    return kinds


# ---- plumbing -------------------------------------------------------------------------

def to_array(t, vals):
    if t == "hge":
        return np.array([[v & M64, (v >> 64) & M64] for v in vals], np.uint64).reshape(-1, 2)
    return np.array(vals, dtype=NPT[t])


def T(G, t):
    return getattr(G, "TYPE_" + t)


def dbat(G, t, vals, hseq=0):
    return G.BAT.from_numpy(T(G, t), to_array(t, vals), hseqbase=hseq, sorted_=False, revsorted=False, key=False,
                            nonil=tnil(t) not in vals)


def obat(O, t, vals, hseq=0):
    return O.Bat.from_array(T(O, t), to_array(t, vals), hseqbase=hseq)


Cst = namedtuple("Cst", "t v")
NAME = {"+": "add", "-": "sub", "*": "mul"}


def dev_calc(G, op, a, b, tp, s1=None, s2=None):
    if isinstance(a, Cst):
        return getattr(G, "BATcalccst" + NAME[op])(a.v, T(G, a.t), b, T(G, tp), s=s1)
    if isinstance(b, Cst):
        return getattr(G, "BATcalc%scst" % NAME[op])(a, b.v, T(G, b.t), T(G, tp), s=s1)
    return getattr(G, "BATcalc" + NAME[op])(a, b, T(G, tp), s1=s1, s2=s2)


def ora_calc(O, op, a, b, tp, s=None):
    if isinstance(a, Cst):
        return O.BATcalc(op, None, b, T(O, tp), s=s, c1=a.v, t1=T(O, a.t))
    if isinstance(b, Cst):
        return O.BATcalc(op, a, None, T(O, tp), s=s, c2=b.v, t2=T(O, b.t))
    return O.BATcalc(op, a, b, T(O, tp), s=s)


def dev_divmod(G, op, a, b, tp):
    if isinstance(a, Cst):
        return G.BATcalcdivmod(op, None, b, T(G, tp), c1=a.v, t1=T(G, a.t))
    if isinstance(b, Cst):
        return G.BATcalcdivmod(op, a, None, T(G, tp), c2=b.v, t2=T(G, b.t))
    return G.BATcalcdivmod(op, a, b, T(G, tp))


def ora_divmod(O, op, a, b, tp):
    if isinstance(a, Cst):
        return O.BATcalcdivmod(op, None, b, T(O, tp), c1=a.v, t1=T(O, a.t))
    if isinstance(b, Cst):
        return O.BATcalcdivmod(op, a, None, T(O, tp), c2=b.v, t2=T(O, b.t))
    return O.BATcalcdivmod(op, a, b, T(O, tp))


def ints(bat):
    return [int(x) for x in bat.values()]


def check_dev(got, want, what):
    assert ints(got) == want.values, what
    s = got.s
    assert (s.count, s.hseqbase, bool(s.tnil), bool(s.tnonil)) == \
        (want.count, want.hseqbase, want.tnil, want.tnonil), what


def text(excinfo):
    return str(excinfo.value).rstrip("\n")


def planted(fx, fy, p, pair, p2=None, pair2=None):
    xs, ys = list(fx), list(fy)
    xs[p], ys[p] = pair
    if p2 is not None:
        assert p2 > p and pair2 != pair
        xs[p2], ys[p2] = pair2
    return xs, ys


def clean_rows(fx, fy, n):
    """n rows of the fitting column (repeated to length)"""
    assert len(fx) > 0
    reps = -(-n // len(fx))
    return (list(fx) * reps)[:n], (list(fy) * reps)[:n]


# ---- CPU: the oracle equals the model ---------------------------------------------------

CPU_CAP = 6000


@pytest.mark.parametrize("t1,t2", PAIRS)
def test_oracle_calc_equals_model(ora, t1, t2):
    for tp in TYPES:
        for op in OPS:
            fx, fy, ovf = split_pairs(op, t1, t2, tp, CPU_CAP)
            assert_reaches_both_ends(op, t1, t2, tp, fx, fy, ovf)
            what = f"{t1}{op}{t2}->{tp}"
            want = model_calc(op, fx, fy, t1, t2, tp, hseqbase=3)
            got = ora_calc(ora, op, obat(ora, t1, fx, 3), obat(ora, t2, fy, 3), tp)
            assert ints(got) == want.values, what
            assert (got.s.count, got.s.hseqbase, bool(got.s.nil), bool(got.s.nonil)) == \
                (want.count, want.hseqbase, want.tnil, want.tnonil), what
            sample = msg_pairs(t1, t2, ovf)
            sample = sample[::max(1, len(sample) // 12)][:12] + [p for _, p in overflow_kinds(op, t1, t2, tp)] \
                if ovf else []
            cx, cy = clean_rows(fx, fy, 9)
            for k, pair in enumerate(sample):
                xs, ys = planted(cx, cy, k % 9, pair)
                with pytest.raises(ModelError) as em:
                    model_calc(op, xs, ys, t1, t2, tp)
                assert em.value.pos == k % 9
                with pytest.raises(ora.OracleError) as eo:
                    ora_calc(ora, op, obat(ora, t1, xs), obat(ora, t2, ys), tp)
                assert text(eo) == str(em.value), (what, pair)


def divmod_columns(t1, t2, tp, cap):
    """dividends x non-zero divisors of the two edge sets, thinned, with +-max
    over +-1, |dividend| < |divisor| and the three nil rows kept"""
    xs = edge_values(t1)
    ys = [y for y in edge_values(t2) if y]
    m1 = tmax(t1)
    keep = [(x, y) for x in (m1, -m1) for y in (1, -1)]
    rest = [(x, y) for x in xs for y in ys]
    step = max(1, -(-len(rest) // cap))
    rows = keep + rest[1::step] + [(tnil(t1), 3), (5, tnil(t2)), (tnil(t1), tnil(t2))]
    assert any(abs(x) < abs(y) for x, y in rows if x != tnil(t1) and y != tnil(t2))
    if t1 == "hge" and t2 == "hge":
        rows += [(tmax("hge"), (1 << 64) + 1), (-(1 << 126) + 1, 3 << 62 << 3), ((1 << 96) + 5, -(1 << 96) - 6)]
        assert any(abs(y) > 1 << 64 and abs(x) >= abs(y) for x, y in rows)
    return [r[0] for r in rows], [r[1] for r in rows]


@pytest.mark.parametrize("t1,t2", PAIRS)
def test_oracle_divmod_equals_model(ora, t1, t2):
    for tp in TYPES:
        xs, ys = divmod_columns(t1, t2, tp, CPU_CAP)
        a, b = obat(ora, t1, xs), obat(ora, t2, ys)
        for op in "/%":
            what = f"{t1}{op}{t2}->{tp}"
            if not divmod_supported(op, t1, t2, tp):
                with pytest.raises(ora.OracleError, match="not supported"):
                    ora_divmod(ora, op, a, b, tp)
                continue
            want = model_divmod(op, xs, ys, t1, t2, tp)
            assert ints(ora_divmod(ora, op, a, b, tp)) == want.values, what
            c = ys[len(ys) // 2]
            assert ints(ora_divmod(ora, op, a, Cst(t2, c), tp)) == model_divmod(op, xs, [c] * len(xs), t1, t2, tp).values
            c = xs[len(xs) // 3]
            assert ints(ora_divmod(ora, op, Cst(t1, c), b, tp)) == model_divmod(op, [c] * len(ys), ys, t1, t2, tp).values
            zs = list(ys)
            zs[4] = 0
            with pytest.raises(ora.OracleError) as eo:
                ora_divmod(ora, op, a, obat(ora, t2, zs), tp)
            assert text(eo) == "22012!division by zero."


def test_model_rounds_like_long_double():
    """the rounded text, where a message has to rely on it"""
    assert fmt_operand("hge", tmax("hge")) == "%d (approx. value)" % (1 << 127)
    assert long_double((1 << 64) + 1) == 1 << 64           # tie to even, down
    assert long_double((1 << 64) + 3) == (1 << 64) + 4     # tie to even, up
    assert long_double(-((1 << 70) + 65)) == -((1 << 70) + 128)
    assert long_double(M64) == M64 and sig_bits(M64 << 60) == 64 and sig_bits((1 << 64) + 1) == 65


# ---- GPU: the device equals the model -------------------------------------------------------

GPU_CAP = 6000


def cst_choices(t):
    b = BITS[t]
    return [tmax(t), -tmax(t), -1, 3, (1 << (b // 2)) + 1, -((tmax(t) + 1) // 2)]


def fitting_with_cst(op, tb, tc, tp, c, cst_first):
    """the BAT's edge values that fit with constant c, and two nil rows"""
    vals = [x for x in edge_values(tb) if abs(exact(op, c, x) if cst_first else exact(op, x, c)) <= tmax(tp)]
    if vals:
        vals = [tnil(tb)] + vals + [tnil(tb)]
    return vals


@pytest.mark.gpu
@pytest.mark.parametrize("t1,t2", PAIRS)
def test_type_sweep(gdk, t1, t2):
    """(a) every triple and operator: BAT o BAT on the fitting column, BAT o
    cst and cst o BAT with edge, max and nil constants"""
    hit_max = 0
    for tp in TYPES:
        for op in OPS:
            what = f"{t1}{op}{t2}->{tp}"
            fx, fy, ovf = split_pairs(op, t1, t2, tp, GPU_CAP)
            assert_reaches_both_ends(op, t1, t2, tp, fx, fy, ovf)
            if (t1, t2, tp, op) == ("lng", "lng", "hge", "*"):   # the unchecked path at its corners
                m = tmax("lng")
                assert (m, m) in zip(fx, fy) and (-m, m) in zip(fx, fy)
            want = model_calc(op, fx, fy, t1, t2, tp, hseqbase=11)
            check_dev(dev_calc(gdk, op, dbat(gdk, t1, fx, 11), dbat(gdk, t2, fy, 11), tp), want, what)
            # constants: t2's with a t1 BAT, then t1's with a t2 BAT
            for tb, tc, first in ((t1, t2, False), (t2, t1, True)):
                ran = 0
                for c in cst_choices(tc):
                    vals = fitting_with_cst(op, tb, tc, tp, c, first)
                    if not vals:
                        continue
                    ran += 1
                    cs = [c] * len(vals)
                    b = dbat(gdk, tb, vals, 5)
                    if first:
                        want = model_calc(op, cs, vals, tc, tb, tp, hseqbase=5)
                        got = dev_calc(gdk, op, Cst(tc, c), b, tp)
                    else:
                        want = model_calc(op, vals, cs, tb, tc, tp, hseqbase=5)
                        got = dev_calc(gdk, op, b, Cst(tc, c), tp)
                    hit_max += c == tmax(tc)
                    check_dev(got, want, (what, "cst", c, first))
                assert ran >= 2, what
                # a nil constant: all nil
                vals = list(edge_values(tb)[:70])
                b = dbat(gdk, tb, vals, 5)
                got = dev_calc(gdk, op, Cst(tc, tnil(tc)), b, tp) if first else dev_calc(gdk, op, b, Cst(tc, tnil(tc)), tp)
                assert ints(got) == [tnil(tp)] * len(vals), what
                s = got.s
                assert (s.count, s.hseqbase, bool(s.tnil), bool(s.tnonil), bool(s.tsorted), bool(s.trevsorted)) == \
                    (len(vals), 5, True, False, True, True), what
    assert hit_max >= 2 * len(TYPES)


EDGE_POS_N = 4099
EDGE_POS = [0, 63, 64, 511, 512, 2047, 2048, EDGE_POS_N - 1]


@pytest.mark.gpu
@pytest.mark.parametrize("t1,t2", PAIRS)
def test_overflow_kinds(gdk, t1, t2):
    """(b) single-overflow columns: the first of two planted pairs is named"""
    cases = 0
    for tp in TYPES:
        for op in OPS:
            fx, fy, ovf = split_pairs(op, t1, t2, tp, GPU_CAP)
            if not ovf:
                continue
            kinds = overflow_kinds(op, t1, t2, tp)
            assert {k for k, _ in kinds} >= {"max+1", "-max-1"}
            full = (t1, t2, tp) in (("lng", "lng", "lng"), ("hge", "hge", "hge"))
            n = EDGE_POS_N if full else 200
            cx, cy = clean_rows(fx, fy, n)
            model_calc(op, cx, cy, t1, t2, tp)   # clean without the planted pairs
            positions = EDGE_POS if full else [1, n - 2]
            for j, (kind, pair) in enumerate(kinds):
                other = next(q for _, q in kinds[j + 1:] + kinds[:j] if q != pair)
                for p in positions:
                    p2 = n - 1 if p < n - 1 else None
                    xs, ys = planted(cx, cy, p, pair, p2, other)
                    with pytest.raises(ModelError) as em:
                        model_calc(op, xs, ys, t1, t2, tp)
                    assert em.value.pos == p
                    expect = "22003!overflow in calculation %s%s%s." % (fmt_operand(t1, pair[0]), op,
                                                                        fmt_operand(t2, pair[1]))
                    assert str(em.value) == expect
                    with pytest.raises(gdk.GDKError) as ed:
                        dev_calc(gdk, op, dbat(gdk, t1, xs), dbat(gdk, t2, ys), tp)
                    assert text(ed) == expect, (f"{t1}{op}{t2}->{tp}", kind, p)
                    cases += 1
    assert cases > 0   # into bte every pair of types can overflow


def subword_values(t, n):
    m = tmax(t)
    return [((i + 1) * 2654435761) % (2 * m + 1) - m for i in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("t", ["bte", "sht", "int"])
def test_subword_slices(gdk, t):
    """(c) ld_any at every byte offset of the 16-byte word, as either operand,
    against an unsliced lng and a constant"""
    w = BITS[t] // 8
    nlo = 16 // w
    sizes = [1, 2, 65, 513]
    parent_vals = subword_values(t, nlo - 1 + max(sizes))
    assert tnil(t) not in parent_vals and len(set(parent_vals[:100])) > 90
    ended_at_last = 0
    for lo in range(nlo):
        for n in sizes:
            for nil_rows in ([(0, n - 1)] if n > 2 else [(0, n - 1), ()]):
                pv = list(parent_vals)
                for r in set(nil_rows):
                    pv[lo + r] = tnil(t)
                parent = dbat(gdk, t, pv)
                sl = gdk.BATslice(parent, lo, lo + n)
                assert sl.count() == n
                ended_at_last += lo + n == len(pv)
                xs = pv[lo:lo + n]
                hs = sl.hseqbase
                ys = [((i * 7) % 23) - 11 for i in range(n)]
                other = dbat(gdk, "lng", ys, hs)
                for op in OPS:
                    what = (t, lo, n, op, nil_rows)
                    check_dev(dev_calc(gdk, op, sl, other, "lng"), model_calc(op, xs, ys, t, "lng", "lng", hs), what)
                    check_dev(dev_calc(gdk, op, other, sl, "lng"), model_calc(op, ys, xs, "lng", t, "lng", hs), what)
                    check_dev(dev_calc(gdk, op, sl, Cst("lng", -3), "lng"),
                              model_calc(op, xs, [-3] * n, t, "lng", "lng", hs), what)
                    check_dev(dev_calc(gdk, op, Cst("lng", 7), sl, "hge"),
                              model_calc(op, [7] * n, xs, "lng", t, "hge", hs), what)
    assert ended_at_last >= 1


def cand_forms(G, n1, n2, r):
    """(name, s1 oids, s2 oids, device s1, device s2): equal counts, positions
    into a (hseqbase 100, n1 rows) and b (hseqbase 7, n2 rows)"""
    k = 300
    o1 = np.sort(r.choice(n1, k, replace=False)).astype(np.uint64) + 100
    o2 = np.sort(r.choice(n2, k, replace=False)).astype(np.uint64) + 7

    def mat(o):
        return G.BAT.from_numpy(G.TYPE_oid, o, sorted_=True, key=True, nonil=True)
    forms = [("oids/oids", o1, o2, mat(o1), mat(o2)),
             ("dense/oids", np.arange(150, 150 + k, dtype=np.uint64), o2, G.BAT.dense(150, k), mat(o2)),
             ("oids/dense", o1, np.arange(9, 9 + k, dtype=np.uint64), mat(o1), G.BAT.dense(9, k))]
    # an except list over a and a mask list over b
    exc = np.sort(r.choice(np.arange(121, 120 + k), 40, replace=False)).astype(np.uint64)
    neg = np.setdiff1d(np.arange(120, 120 + k + 40, dtype=np.uint64), exc)
    bits = np.zeros(n2 - 5, bool)
    bits[r.choice(n2 - 5, k, replace=False)] = True
    msk = (np.flatnonzero(bits) + 10).astype(np.uint64)
    forms.append(("except/mask", neg, msk, G.BAT.negoid_cand(120, k, exc), G.BAT.mask_cand(10, bits)))
    for name, a, b, sa, sb in forms:
        assert len(a) == len(b) == k and not np.array_equal(a - 100, b - 7), name
        assert sa.hseqbase == 0 and sb.hseqbase == 0
        assert np.array_equal(G.cand_oids(sa), a) and np.array_equal(G.cand_oids(sb), b), name
    return forms


@pytest.mark.gpu
@pytest.mark.parametrize("t1,t2,tp", [("sht", "lng", "lng"), ("hge", "int", "hge")])
def test_two_candidate_lists(gdk, t1, t2, tp):
    """(d) a[s1[i] - 100] op b[s2[i] - 7] with s1 != s2, through the slow kernel
    k_calc"""
    r = np.random.default_rng(77)
    n1, n2 = 700, 650
    av = [int(v) for v in r.integers(-30000, 30000, n1)]
    mul_ok = tmax(tp) // 30000   # a product of the two ranges fits
    bv = [int(v) for v in r.integers(-min(tmax(t2), mul_ok, 10 ** 9), min(tmax(t2), mul_ok, 10 ** 9), n2)]
    for i in range(0, n1, 37):
        av[i] = tnil(t1)
    for i in range(5, n2, 41):
        bv[i] = tnil(t2)
    A, B = dbat(gdk, t1, av, 100), dbat(gdk, t2, bv, 7)
    forms = cand_forms(gdk, n1, n2, r)
    for name, o1, o2, s1, s2 in forms:
        xs = [av[int(o) - 100] for o in o1]
        ys = [bv[int(o) - 7] for o in o2]
        for op in OPS:
            check_dev(dev_calc(gdk, op, A, B, tp, s1, s2), model_calc(op, xs, ys, t1, t2, tp, hseqbase=0),
                      (name, op))
    # overflow in candidate order, on the operand that has the result's type:
    # +-big times any partner beyond +-1 leaves the range
    big = tmax("lng") - 1 if tp == "lng" else (1 << 127) - (1 << 63)
    name, o1, o2, s1, s2 = forms[0]
    in_b = t2 == tp

    def run(work):
        """(device operands, model operands) with `work` in place of the big side"""
        a2, b2 = (av, work) if in_b else (work, bv)
        return (dbat(gdk, t1, a2, 100), dbat(gdk, t2, b2, 7),
                [a2[int(o) - 100] for o in o1], [b2[int(o) - 7] for o in o2])

    side, oids, base = (bv, o2, 7) if in_b else (av, o1, 100)
    others, ooids, obase, ot = (av, o1, 100, t1) if in_b else (bv, o2, 7, t2)
    cands = set(int(o) for o in oids)
    skipped = next(i for i in range(base, base + len(side)) if i not in cands)
    work = list(side)
    work[skipped - base] = big          # would overflow, but is no candidate
    A2, B2, xs, ys = run(work)
    check_dev(dev_calc(gdk, "*", A2, B2, tp, s1, s2), model_calc("*", xs, ys, t1, t2, tp), "non-candidate")
    # two overflowing candidates: the earlier one is named
    usable = [i for i in range(len(oids)) if abs(others[int(ooids[i]) - obase]) > 1
              and others[int(ooids[i]) - obase] != tnil(ot)]
    i1, i2 = usable[len(usable) // 3], usable[2 * len(usable) // 3]
    assert i1 < i2
    work[int(oids[i1]) - base] = big
    work[int(oids[i2]) - base] = -big
    A2, B2, xs, ys = run(work)
    with pytest.raises(ModelError) as em:
        model_calc("*", xs, ys, t1, t2, tp)
    assert em.value.pos == i1
    assert str(em.value) == "22003!overflow in calculation %s*%s." % (fmt_operand(t1, xs[i1]), fmt_operand(t2, ys[i1]))
    with pytest.raises(gdk.GDKError) as ed:
        dev_calc(gdk, "*", A2, B2, tp, s1, s2)
    assert text(ed) == str(em.value)
    # unequal candidate counts
    short = gdk.BAT.from_numpy(gdk.TYPE_oid, o2[:-1], sorted_=True, key=True, nonil=True)
    with pytest.raises(gdk.GDKError, match="inputs not the same size"):
        dev_calc(gdk, "+", A, B, tp, s1, short)


@pytest.mark.gpu
def test_second_grid_sweep(gdk):
    """(e) past the grid cap of 4096 blocks x 2048 rows the wave loop runs a
    second time: lng + lng -> lng, nils in the last partial chunk, and the
    only overflow in the second sweep.  The model is numpy here (the values
    are small, no sum comes near the range), for the size alone."""
    n = 2048 * 4096 + 513
    a = (np.arange(n, dtype=np.int64) * 7919) % 100003 - 50000
    b = (np.arange(n, dtype=np.int64) * 104729) % 99991 - 49000
    nil = tnil("lng")
    a[n - 500] = nil
    b[n - 3] = nil
    a[n - 1] = nil
    b[n - 1] = nil
    a[12345] = nil
    A = gdk.BAT.from_numpy(gdk.TYPE_lng, a, nonil=False, sorted_=False, revsorted=False, key=False)
    B = gdk.BAT.from_numpy(gdk.TYPE_lng, b, nonil=False, sorted_=False, revsorted=False, key=False)
    isn = (a == nil) | (b == nil)
    want = np.where(isn, nil, a + b)
    assert np.abs(a[~isn]).max() < 1 << 20 and np.abs(b[~isn]).max() < 1 << 20
    got = gdk.BATcalcadd(A, B, gdk.TYPE_lng)
    gv = got.to_numpy()
    assert np.array_equal(gv, want)
    assert int((gv == nil).sum()) == 4 == int(isn.sum())
    assert (got.s.count, bool(got.s.tnil), bool(got.s.tnonil)) == (n, True, False)
    del got, gv
    p = 2048 * 4096 + 100
    assert not isn[p] and b[p] > 5
    a[p] = tmax("lng") - 5
    A = gdk.BAT.from_numpy(gdk.TYPE_lng, a, nonil=False, sorted_=False, revsorted=False, key=False)
    with pytest.raises(gdk.GDKError) as ed:
        gdk.BATcalcadd(A, B, gdk.TYPE_lng)
    assert text(ed) == "22003!overflow in calculation %d+%d." % (tmax("lng") - 5, b[p])


@pytest.mark.gpu
@pytest.mark.parametrize("t1,t2", PAIRS)
def test_divmod_edges(gdk, t1, t2):
    """(f) every supported integer / and % triple, three forms"""
    ran = wrapped = 0
    for tp in TYPES:
        xs, ys = divmod_columns(t1, t2, tp, GPU_CAP)
        a, b = dbat(gdk, t1, xs, 4), dbat(gdk, t2, ys, 4)
        for op in "/%":
            what = f"{t1}{op}{t2}->{tp}"
            if not divmod_supported(op, t1, t2, tp):
                with pytest.raises(gdk.GDKError, match="not supported"):
                    dev_divmod(gdk, op, a, b, tp)
                continue
            ran += 1
            if op == "%" and RANK[tp] < RANK[t1]:
                wrapped += any(wrap(tp, x) != x for x in xs if x != tnil(t1))
            want = model_divmod(op, xs, ys, t1, t2, tp, hseqbase=4)
            got = dev_divmod(gdk, op, a, b, tp)
            assert ints(got) == want.values, what
            assert (got.s.count, got.s.hseqbase) == (want.count, 4), what
            for c in (ys[len(ys) // 2], 1, -1, tmax(t2)):
                got = dev_divmod(gdk, op, a, Cst(t2, c), tp)
                assert ints(got) == model_divmod(op, xs, [c] * len(xs), t1, t2, tp).values, (what, "cst", c)
            for c in (xs[len(xs) // 3], tmax(t1), -tmax(t1), 1):
                got = dev_divmod(gdk, op, Cst(t1, c), b, tp)
                assert ints(got) == model_divmod(op, [c] * len(ys), ys, t1, t2, tp).values, (what, "cst first", c)
    assert ran >= 2
    if RANK[t1] > 0:
        assert wrapped or RANK[t2] >= RANK[t1]


@pytest.mark.gpu
@pytest.mark.parametrize("op,t1,t2,tp", [("/", "lng", "lng", "lng"), ("%", "hge", "int", "int")])
def test_division_by_zero_positions(gdk, op, t1, t2, tp):
    n = EDGE_POS_N
    xs = [(i * 7919) % 1000 - 500 for i in range(n)]
    ys = [(i % 13) + 1 for i in range(n)]
    a = dbat(gdk, t1, xs)
    assert ints(dev_divmod(gdk, op, a, dbat(gdk, t2, ys), tp)) == model_divmod(op, xs, ys, t1, t2, tp).values
    for p in EDGE_POS:
        zs = list(ys)
        zs[p] = 0
        with pytest.raises(ModelError) as em:
            model_divmod(op, xs, zs, t1, t2, tp)
        assert em.value.pos == p and str(em.value) == "22012!division by zero."
        with pytest.raises(gdk.GDKError) as ed:
            dev_divmod(gdk, op, a, dbat(gdk, t2, zs), tp)
        assert text(ed) == "22012!division by zero.", p


@pytest.mark.gpu
def test_divmod_unsupported_text(gdk, ora):
    """five refused triples: the device's text is the oracle's"""
    for op, t1, t2, tp in [("/", "int", "int", "bte"), ("/", "hge", "bte", "lng"), ("/", "lng", "lng", "int"),
                           ("%", "int", "sht", "bte"), ("%", "hge", "lng", "int")]:
        assert not divmod_supported(op, t1, t2, tp)
        xs, ys = [5, 7, -9], [1, 2, 3]
        with pytest.raises(ora.OracleError) as eo:
            ora_divmod(ora, op, obat(ora, t1, xs), obat(ora, t2, ys), tp)
        with pytest.raises(gdk.GDKError) as ed:
            dev_divmod(gdk, op, dbat(gdk, t1, xs), dbat(gdk, t2, ys), tp)
        assert "not supported" in text(ed) and text(ed) == text(eo), (op, t1, t2, tp)
