"""The references of test_select_groupsum_star.py pinned on the CPU: the model
in plain Python integers against the star chain through the oracle's
operators (two BATprojects per gathered column, BATproject(p, c) after a
predicate on one), on every case the GPU tests use."""
import pytest

import star_ref as S

CASES = S.generated_cases()


def agree(ora, case):
    want, live, gathers, lines = S.model(case)
    # operands from +-2^40: the overflow rule alone never declines a generated case
    assert S.in_scope(case, live)
    assert S.ora_chain(ora, case) == want
    return want


@pytest.mark.parametrize("cid", list(CASES))
def test_model_is_the_oracle_chain(ora, cid):
    case = CASES[cid]()
    agree(ora, case)


def test_cases_hold_what_they_claim():
    """Nil oids reach predicates, keys and factors; the dimension's hseqbase matters."""
    case = S.star_case(2_049, "two_dims")
    _, _, nil = S.gathered(case)
    assert 20 < nil["A.ak"].sum() < 80 and case.dims["A"]["hseq"] == 1000
    want, live, gathers, _ = S.model(case)
    assert any(g["keys"][1] == S.tnil("int") for g in want)              # a nil key group from a nil oid
    assert any(nn < g["count"] for g in want for nn in g["nonnil"])      # nil terms
    assert 0 < gathers < 6 * case.n
    shifted = S.Case(case.fact, {"A": dict(case.dims["A"], hseq=1001), "B": case.dims["B"]}, case.routes,
                     case.preds, case.keys, case.sums)
    with pytest.raises(S.BadOid):                                        # oid 1000 is below the dimension now
        S.model(shifted)


def test_merge_case(ora):
    case = S.merge_case()
    want = agree(ora, case)
    assert len(want) == 200


@pytest.mark.parametrize("kind", ["beyond", "below"])
@pytest.mark.parametrize("where", ["pred", "key", "factor"])
def test_bad_oid_raises_only_where_it_survives(ora, where, kind):
    live_case = S.bad_oid_case(where, removed=False, kind=kind)
    with pytest.raises(S.BadOid):
        S.model(live_case)
    with pytest.raises(ora.OracleError, match="does not match always"):
        S.ora_chain(ora, live_case)
    agree(ora, S.bad_oid_case(where, removed=True, kind=kind))


def test_overflow_cases(ora):
    case = S.overflow_case(reached=False)
    want, live, _, _ = S.model(case)
    assert S.in_scope(case, live) and S.ora_chain(ora, case) == want
    case = S.overflow_case(reached=True)
    _, live, _, _ = S.model(case)
    assert not S.in_scope(case, live)
    with pytest.raises(ora.OracleError):
        S.ora_chain(ora, case)


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("form", list(S.NIL_FORMS))
def test_null_foreign_key_filters(ora, form, first):
    """IS NULL, IS NOT NULL and range(nil, nil) on a gathered column whose dimension holds no nil: the nil
    oids' rows are the ones IS NULL keeps and the others drop."""
    case = S.null_fk_case(form, first)
    want = agree(ora, case)
    _, live, _, _ = S.model(case)
    nil = case.fact["va"][1] == S.np.uint64(S.OID_NIL)
    assert 10 < nil.sum() < 100 and len(want) == 3
    assert (nil[live]).all() if form == "isnull" else not nil[live].any()
    with pytest.raises(S.BadOid):
        S.model(S.null_fk_case(form, first, bad=True))
    with pytest.raises(ora.OracleError, match="does not match always"):
        S.ora_chain(ora, S.null_fk_case(form, first, bad=True))


def test_no_row_left_after_a_gathered_predicate(ora):
    assert agree(ora, S.empty_after_gather_case(bad=False)) == []
    with pytest.raises(ora.OracleError, match="does not match always"):
        S.ora_chain(ora, S.empty_after_gather_case(bad=True))
