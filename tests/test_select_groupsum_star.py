"""gdk.select_groupsum_star: the fused select cascade + GROUP BY sums with
columns of dimension tables gathered through join indexes, against three
references that must agree bit for bit -- the star chain through the oracle's
operators, through the device operators (fused=False), and a model in plain
Python integers (star_ref.py; test_star_model.py pins the first and the last
on the CPU)."""
import functools

import numpy as np
import pytest

import star_ref as S
import test_select_groupsum_hash as H

CASES = S.generated_cases()


@functools.lru_cache(maxsize=None)
def reference(cid):
    case = CASES[cid]()
    return case, S.model(case)


def errbuf_clean_none(gdk, *args, **kw):
    """fallback=False answers None and leaves no error text."""
    gdk.lib().mgdk_GDKclrerr()
    assert gdk.select_groupsum_star(*args, fallback=False, **kw) is None
    assert gdk.lib().mgdk_GDKerrbuf() == b""


def check_all(gdk, ora, case, want=None, override=None, oenv=None):
    """Model == oracle chain == device operators == fused (which must have run)."""
    want = S.model(case) if want is None else want
    groups, live, gathers, lines = want
    assert S.in_scope(case, live)
    assert S.ora_chain(ora, case, oenv) == groups
    gp, gk, gs, vias, s = S.request(case, *S.bind(gdk, case, override), gdk)
    got, used = gdk.select_groupsum_star(gp, gk, gs, vias, s, fused=False)
    assert not used and got == groups
    got, used = gdk.select_groupsum_star(gp, gk, gs, vias, s, fused=True, fallback=False)
    assert used, "an in-scope request was declared not applicable"
    assert got == groups
    assert gdk.select_groupsum_star_last_gathers() == gathers
    return groups


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_generated(gdk, ora, cid):
    """A gathered column as first predicate, later predicate, first and second key, factor plain
    and under cst - col; dimension widths 1, 2, 4, 8; two dimensions; one dimension column
    through two routes; nil oids at 2 % in every join index; fact rows around the chunk and
    workgroup edges; dimensions of 1 .. 70 000 rows at hseqbase 0 and 1000; a dense candidate
    list starting mid-column (the guarded loads cover the join index and the gather)."""
    case, want = reference(cid)
    check_all(gdk, ora, case, want)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [257, 70_001])
def test_no_vias_is_the_hashed_entry(gdk, n):
    cols = H.make_case(n)
    gp, gk, gs = H.bound(H.bind(gdk, cols), H.PREDS, H.KEY_FORMS["bte_int"], H.SUMS)
    want = gdk.select_groupsum_hash(gp, gk, gs, fallback=False)
    assert want is not None and want == (H.case_model(n, "bte_int")[0], True)
    assert gdk.select_groupsum_star(gp, gk, gs, [], fallback=False) == want
    assert gdk.select_groupsum_star_last_lines() == gdk.select_groupsum_hash_last_lines()
    assert gdk.select_groupsum_star_last_gathers() == 0
    assert gdk.select_groupsum_star(gp, gk, gs, [], fused=False) == (want[0], False)


@pytest.mark.gpu
def test_merge_across_workgroups(gdk, ora):
    want = check_all(gdk, ora, S.merge_case())
    assert len(want) == 200


@pytest.mark.gpu
def test_str_key_through_a_join_index(gdk, ora):
    """A str dimension column (two-byte offsets, a heap below 64 KiB) as a key; a nil oid into
    it is refused by the operators' projection, so the fused entry declines."""
    from strheap import build_heap, tail
    n, dn = 2_049, 60
    r = np.random.default_rng(41)
    heap, offs = build_heap([b"nation%04d" % i for i in range(40)], 1)
    rel = np.array([offs[w][0] for w in r.integers(0, 40, dn)])
    assert rel.max() > 255 and len(heap) < 1 << 16
    va = (r.integers(0, dn, n) + 5).astype(np.uint64)
    fact = {"p0": ("int", H.filtered_p0(n)), "va": ("oid", va),
            "v4": ("int", r.integers(-1000, 1000, n).astype(np.int32))}
    dims = {"A": dict(hseq=5, cols={"as": ("int", rel.astype(np.int32))})}     # model and oracle: the offsets
    case = S.Case(fact, dims, {"A.as": ("A", "as", "va")}, [S.P0], ["A.as"], [("v4",)])
    sbat = gdk.BAT.from_numpy(gdk.TYPE_str, tail(rel, 2), hseqbase=5, vheap=heap, sorted_=False, revsorted=False,
                              key=False, nonil=False)
    assert sbat.s.twidth == 2
    want = check_all(gdk, ora, case, override={("A", "as"): sbat})
    assert len(want) == len(set(rel.tolist()))
    va = va.copy()
    va[10] = S.OID_NIL
    assert fact["p0"][1][10] == 10
    case = S.Case(dict(fact, va=("oid", va)), dims, case.routes, case.preds, case.keys, case.sums)
    errbuf_clean_none(gdk, *S.request(case, *S.bind(gdk, case, {("A", "as"): sbat}), gdk))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["beyond", "below"])
@pytest.mark.parametrize("where", ["pred", "key", "factor"])
def test_bad_oid(gdk, ora, where, kind):
    """An oid that no row of the dimension has: on a live row the fused entry declines without
    an error text and the operators raise theirs; on a row an earlier predicate removed it
    decides nothing and the request is fused."""
    case = S.bad_oid_case(where, removed=False, kind=kind)
    req = S.request(case, *S.bind(gdk, case), gdk)
    errbuf_clean_none(gdk, *req)
    with pytest.raises(ora.OracleError) as oe:
        S.ora_chain(ora, case)
    with pytest.raises(gdk.GDKError) as ge:
        gdk.select_groupsum_star(*req)
    assert str(ge.value) == str(oe.value)
    with pytest.raises(gdk.GDKError):
        gdk.select_groupsum_star(*req, fused=False)
    check_all(gdk, ora, S.bad_oid_case(where, removed=True, kind=kind))


@pytest.mark.gpu
def test_gathers_are_late(gdk):
    """last_gathers is, per use, the rows live at that step whose oid is not nil -- a dead row
    loads nothing; last_lines counts the join index as an 8-byte column at its first use."""
    n, dn = 262_144, 2_500
    r = np.random.default_rng(11)
    first = np.arange(n, dtype=np.int32)                       # sorted: one contiguous 10 % survives
    va = r.integers(0, dn, n).astype(np.uint64)
    vb = r.integers(0, 40, n).astype(np.uint64)
    va[r.random(n) < 0.02] = S.OID_NIL
    fact = {"first": ("int", first), "va": ("oid", va), "vb": ("oid", vb),
            "x": ("lng", r.integers(1, 1 << 30, n).astype(np.int64))}
    dims = {"A": dict(hseq=0, cols={"year": ("sht", (1992 + np.arange(dn) // 366).astype(np.int16)),
                                    "w": ("int", r.integers(-100, 100, dn).astype(np.int32))}),
            "B": dict(hseq=0, cols={"nat": ("int", (np.arange(40) % 25).astype(np.int32))})}
    routes = {"A.year": ("A", "year", "va"), "A.w": ("A", "w", "va"), "B.nat": ("B", "nat", "vb")}
    lo, hi = n // 3, n // 3 + n // 10
    preds = [("first", lo, hi, True, False, False), ("A.year", 1995, "<=")]
    case = S.Case(fact, dims, routes, preds, ["B.nat"], [("x", "A.w"), ("x",)])
    groups, live, gathers, lines = S.model(case)
    m1 = (first >= lo) & (first < hi)
    year = dims["A"]["cols"]["year"][1]
    nil = va == np.uint64(S.OID_NIL)
    assert (live == (m1 & ~nil & (year[np.where(nil, 0, va).astype(np.int64)] <= 1995))).all()
    assert gathers == int((m1 & ~nil).sum()) + 2 * int(live.sum())          # year; nat and w
    assert lines == (H.lines_touched(m1, 8) + H.lines_touched(live, 8) + H.lines_touched(live, 8))   # va, vb, x
    req = S.request(case, *S.bind(gdk, case), gdk)
    assert gdk.select_groupsum_star(*req, fallback=False) == (groups, True)
    assert gdk.select_groupsum_star_last_gathers() == gathers
    assert gdk.select_groupsum_star_last_lines() == lines
    assert gathers < 3 * n // 5 and lines < 3 * 8 * n // 128 // 5               # far below every row


@pytest.mark.gpu
def test_overflow_is_decided_by_the_gathered_values(gdk, ora):
    """The minima and maxima are those of the values the survivors gather: 2^62 in a dimension
    row that no survivor reaches decides nothing; reached, cst + col leaves lng and the request
    stays with the operators, which raise."""
    check_all(gdk, ora, S.overflow_case(reached=False))
    case = S.overflow_case(reached=True)
    req = S.request(case, *S.bind(gdk, case), gdk)
    errbuf_clean_none(gdk, *req)
    with pytest.raises(ora.OracleError) as oe:
        S.ora_chain(ora, case)
    with pytest.raises(gdk.GDKError) as ge:
        gdk.select_groupsum_star(*req)
    assert str(ge.value) == str(oe.value)


@pytest.mark.gpu
@pytest.mark.parametrize("why", ["via_not_oid", "via_other_count", "seventeen_vias", "materialised_candidates"])
def test_out_of_scope_answers_cleanly(gdk, why):
    case = S.star_case(2_049, "key0")
    env, vias = S.bind(gdk, case)
    gp, gk, gs, vias, s = S.request(case, env, vias, gdk)
    if why == "via_not_oid":
        vias = [(vias[0][0], gdk.BAT.from_numpy(gdk.TYPE_lng, case.fact["va"][1].astype(np.int64)))]
    elif why == "via_other_count":
        vias = [(vias[0][0], gdk.BAT.from_numpy(gdk.TYPE_oid, case.fact["va"][1][:-1].copy()))]
    elif why == "seventeen_vias":
        vias = vias + [(gdk.BAT.from_numpy(gdk.TYPE_int, np.arange(3, dtype=np.int32)), env["va"]) for _ in range(16)]
    else:
        s = gdk.BAT.from_numpy(gdk.TYPE_oid, np.arange(0, case.n, 2, dtype=np.uint64))
    errbuf_clean_none(gdk, gp, gk, gs, vias, s)


@pytest.mark.gpu
@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("form", list(S.NIL_FORMS))
def test_null_foreign_key_filters(gdk, ora, form, first):
    """IS NULL, IS NOT NULL and range(nil, nil) on a gathered column: the dimension column holds no nil and
    says so, the gathered values hold one per nil oid.  The predicate is scanned -- fused, equal to the
    references -- and a bad oid on a live row under it declines the request."""
    case = S.null_fk_case(form, first)
    env, vias = S.bind(gdk, case)
    assert env["A.a4"].s.tnonil and not env["va"].s.tnonil
    want = check_all(gdk, ora, case)
    assert len(want) == 3
    bad = S.null_fk_case(form, first, bad=True)
    req = S.request(bad, *S.bind(gdk, bad), gdk)
    errbuf_clean_none(gdk, *req)
    with pytest.raises(gdk.GDKError, match="does not match always"):
        gdk.select_groupsum_star(*req)


@pytest.mark.gpu
def test_no_row_left_after_a_gathered_predicate(gdk, ora):
    """A predicate no row can pass after a gathered one: the operators still project for the gathered
    predicate, so the fused entry leaves the request to them -- no groups, or their error for a bad oid."""
    case = S.empty_after_gather_case(bad=False)
    assert S.ora_chain(ora, case) == []
    req = S.request(case, *S.bind(gdk, case), gdk)
    errbuf_clean_none(gdk, *req)
    assert gdk.select_groupsum_star(*req) == ([], False)
    bad = S.empty_after_gather_case(bad=True)
    req = S.request(bad, *S.bind(gdk, bad), gdk)
    errbuf_clean_none(gdk, *req)
    with pytest.raises(gdk.GDKError, match="does not match always"):
        gdk.select_groupsum_star(*req)
    # the empty predicate first: no row reaches the projection, in either path
    case = S.Case(bad.fact, bad.dims, bad.routes, [bad.preds[2], bad.preds[1]], bad.keys, bad.sums)
    assert S.ora_chain(ora, case) == []
    assert gdk.select_groupsum_star(*S.request(case, *S.bind(gdk, case), gdk), fallback=False) == ([], True)
