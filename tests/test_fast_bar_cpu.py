"""The tolerance-mode bar (tests/test_gpu_full_fast.py) on synthetic arrays, without a GPU: a NaN or an
infinity on one side only fails it, the same non-finite class on both sides passes, and on finite values
the bar is the relative 1e-4 it always was."""
from types import SimpleNamespace

import numpy as np
import pytest

from helpers import finite_parts, nonfinite_mismatch
from test_gpu_full_fast import (FORCE_RTOL, check_fast, check_fast_position, check_fast_velocity,
                                fast_against_exact)

INF, NAN = np.float32(np.inf), np.float32(np.nan)
P = SimpleNamespace(full_cell_inv=10.0)          # a cell edge of 0.1: the position bar is 1e-7 + 2 ulps
DT = 1e-3


def vec(rows):
    return np.ascontiguousarray(np.asarray(rows, np.float32).reshape(-1))


def step(acc, rho=None, ncount=None):
    n = np.asarray(acc).size // 3
    rho = np.ones(n, np.float32) if rho is None else np.asarray(rho, np.float32)
    ncount = np.full(n, 5, np.int32) if ncount is None else ncount
    return SimpleNamespace(mAcceleration=vec(acc), mDensity=rho, mNeighborCount=ncount)


def ref_of(part):
    return dict(acc=part.mAcceleration.copy(), rho=part.mDensity.copy(), ncount=part.mNeighborCount.copy())


BASE = [[1.0, 2.0, 3.0], [-0.5, 0.25, 4.0], [7.0, -1.0, 0.0]]

# (got, want) pairs in row 1, component 0
MISMATCH = [("nan vs finite", NAN, np.float32(1.0)),
            ("finite vs nan", np.float32(1.0), NAN),
            ("+inf vs -inf", INF, -INF),
            ("+inf vs finite", INF, np.float32(3.0e38)),
            ("-inf vs finite", -INF, np.float32(-1.0)),
            ("nan vs +inf", NAN, INF)]
MATCH = [("nan vs nan", NAN, NAN), ("+inf vs +inf", INF, INF), ("-inf vs -inf", -INF, -INF),
         ("nan vs nan of another payload", NAN, -np.float32(np.nan))]


def with_component(rows, value):
    a = np.array(rows, np.float32)
    a[1, 0] = value
    return a


@pytest.mark.parametrize("name,got,want", MISMATCH, ids=[m[0] for m in MISMATCH])
def test_a_nonfinite_component_of_another_class_fails_every_bar(name, got, want):
    a, b = with_component(BASE, got), with_component(BASE, want)
    assert nonfinite_mismatch(a, b).sum() == 1
    with pytest.raises(AssertionError, match="non-finite class"):
        check_fast(step(a), ref_of(step(b)), P, None, name)
    with pytest.raises(AssertionError, match="non-finite class"):
        check_fast(step(a), ref_of(step(b)), P, None, name, scale=lambda: np.ones(3))   # the clause too
    with pytest.raises(AssertionError, match="non-finite class"):
        check_fast_velocity(vec(a), vec(b), np.ones(3), DT, name)
    with pytest.raises(AssertionError, match="non-finite class"):
        check_fast_position(vec(a), vec(b), P, name)
    with pytest.raises(AssertionError, match="non-finite class"):
        fast_against_exact(vec(a), vec(b), name)


@pytest.mark.parametrize("name,got,want", MATCH, ids=[m[0] for m in MATCH])
def test_the_same_nonfinite_class_on_both_sides_passes(name, got, want):
    a, b = with_component(BASE, got), with_component(BASE, want)
    assert not nonfinite_mismatch(a, b).any()
    worst, allowed = check_fast(step(a), ref_of(step(b)), P, None, name)
    assert worst == 0.0 and np.isfinite(allowed).all()
    check_fast_velocity(vec(a), vec(b), allowed, DT, name)
    check_fast_position(vec(a), vec(b), P, name)
    assert fast_against_exact(vec(a), vec(b), name).max() == 0.0


def test_the_finite_components_of_a_partly_nonfinite_row_still_meet_the_bar():
    """(nan, y, z) against (nan, y', z'): y and z are held to the bar (the skip branch's componentwise
    NaN of a particle at x = inf; its position keeps finite y and z)"""
    a = np.array(BASE, np.float32)
    a[1, 0] = NAN
    b = a.copy()
    b[1, 2] *= np.float32(1.01)
    with pytest.raises(AssertionError, match="force rel err"):
        check_fast(step(a), ref_of(step(b)), P, None)
    with pytest.raises(AssertionError, match="velocity"):
        check_fast_velocity(vec(a), vec(b), np.zeros(3), DT)
    with pytest.raises(AssertionError, match="position"):
        check_fast_position(vec(a), vec(b), P)
    with pytest.raises(AssertionError, match="beyond 1e-4 of the exact mode"):
        fast_against_exact(vec(a), vec(b))


def test_densities_nan_on_one_side_only_fail_and_on_both_pass():
    acc = np.array(BASE, np.float32)
    rho = np.array([1.0, NAN, 2.0], np.float32)
    check_fast(step(acc, rho), ref_of(step(acc, rho)), P, None)
    with pytest.raises(AssertionError, match="density"):
        check_fast(step(acc, rho), ref_of(step(acc, np.nan_to_num(rho))), P, None)


def old_vec_rel(a, b):
    """the bar's relative error as it was computed before the non-finite rule"""
    a = np.asarray(a, np.float64).reshape(-1, 3)
    b = np.asarray(b, np.float64).reshape(-1, 3)
    num = np.linalg.norm(a - b, axis=1)
    den = np.maximum(np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1))
    den[den == 0] = 1.0
    return num / den


def test_before_the_rule_a_nan_passed_the_bar():
    """what the rule closes: a NaN row's relative error is NaN, and NaN > 1e-4 is False"""
    a, b = with_component(BASE, NAN), np.array(BASE, np.float32)
    rel = old_vec_rel(a, b)
    assert np.isnan(rel[1]) and not (rel > FORCE_RTOL).any()


def test_the_1e_4_edge_is_where_it_was():
    """finite values: the same verdict and the same allowed force as the formulas before the rule -
    exactly at the edge and on random rows spread around it"""
    b = np.array([[1.0, 0.0, 0.0]], np.float32)
    at = np.array([[1.0 - 2.0 ** -14, 0.0, 0.0]], np.float32)     # 6.1e-5 relative: passes
    past = np.array([[1.0 - 2.0 ** -13, 0.0, 0.0]], np.float32)   # 1.22e-4 relative: fails
    check_fast(step(at), ref_of(step(b)), P, None)
    with pytest.raises(AssertionError, match="force rel err"):
        check_fast(step(past), ref_of(step(b)), P, None)
    rng = np.random.default_rng(5)
    verdicts = []
    for _ in range(200):
        want = rng.normal(size=(64, 3)).astype(np.float32)
        got = (want * (1.0 + rng.normal(scale=0.4e-4, size=(64, 1)))).astype(np.float32)
        old = old_vec_rel(got, want)
        fails = bool((old > FORCE_RTOL).any())
        verdicts.append(fails)
        if fails:
            with pytest.raises(AssertionError):
                check_fast(step(got), ref_of(step(want)), P, None)
            continue
        worst, allowed = check_fast(step(got), ref_of(step(want)), P, None)
        assert worst == old.max()
        g, w = got.astype(np.float64), want.astype(np.float64)
        assert np.array_equal(allowed, FORCE_RTOL * np.maximum(np.linalg.norm(g, axis=1), np.linalg.norm(w, axis=1)))
    assert 20 < sum(verdicts) < 180          # both verdicts were tried


def test_finite_parts_leaves_finite_rows_alone():
    a = np.array(BASE, np.float32)
    b = a * np.float32(1.5)
    x, y = finite_parts(a, b)
    assert np.array_equal(x, a.astype(np.float64)) and np.array_equal(y, b.astype(np.float64))
