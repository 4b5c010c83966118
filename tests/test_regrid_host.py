"""``jdi.regrid_plan`` (picaso_amd/regrid.py) and ``jdi.mean_regrid`` against tests/golden/regrid.npz -- arrays the
reference's own ``mean_regrid`` / ``create_grid`` produced (tests/golden/make_regrid.py; reference justplotit.py:31-63).  The
plan finds every bin as ONE contiguous column range once per grid; its centres, its counts and the ranges themselves must
be the reference's binning, edge cases included (columns on an edge, the closed last edge, columns outside, empty bins).
No GPU: the plan uploads nothing until a spectrum uses it."""
import importlib.util
import os

import numpy as np
import pytest

from helpers import GOLDEN

_spec = importlib.util.spec_from_file_location("make_regrid", os.path.join(GOLDEN, "make_regrid.py"))
make_regrid = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_regrid)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "regrid.npz"))


@pytest.mark.parametrize("name", make_regrid.CASES)
def test_fixture_inputs_are_rebuilt_bit_for_bit(gold, name):
    x, y, newx, R = make_regrid.case(name)
    assert y.shape == (make_regrid.NROWS, x.size)
    assert np.array_equal(y[:, ::97], gold[name + "/y_probe"], equal_nan=True)


@pytest.mark.parametrize("name", make_regrid.CASES)
def test_plan_centres_counts_and_ranges(gold, name):
    from picaso_amd import justdoit as jdi
    x, y, newx, R = make_regrid.case(name)
    plan = jdi.regrid_plan(x, newx=newx, R=R)
    assert plan.nbins == len(gold[name + "/centres"]) and plan.nwno == x.size
    assert np.array_equal(plan.centres, gold[name + "/centres"])
    assert np.array_equal(plan.counts, gold[name + "/counts"])
    assert np.array_equal(plan.edges, gold[name + "/edges"])
    assert plan.start.dtype == np.int32 and plan.start.shape == (plan.nbins + 1,)
    assert np.all(np.diff(plan.start) >= 0) and plan.start[0] >= 0 and plan.start[-1] <= x.size
    assert np.array_equal(np.diff(plan.start), plan.counts)
    # the ranges are the reference's bins, column by column: [e_j, e_j+1), the last one closed, the rest in no bin
    e = gold[name + "/edges"]
    member = np.full(x.size, -1)
    for j in range(plan.nbins):
        member[plan.start[j]:plan.start[j + 1]] = j
    for i, xv in enumerate(x):
        inside = [j for j in range(plan.nbins) if e[j] <= xv < e[j + 1] or (j == plan.nbins - 1 and xv == e[-1])]
        assert member[i] == (inside[0] if inside else -1), (name, i)


def test_edge_cases_of_case_d_are_what_the_issue_says(gold):
    x, _, newx, _ = make_regrid.case("D")
    from picaso_amd import justdoit as jdi
    plan = jdi.regrid_plan(x, newx=newx)
    assert list(plan.edges) == [5.5, 15.5, 25.5, 35.5]
    assert list(x[plan.start]) == [5.5, 15.5, 25.5] + [36.0]        # columns ON every edge; 35.5 belongs to the last bin
    assert list(plan.counts) == [20, 20, 21]
    c = gold["C/counts"]
    assert (c == 0).sum() > 100 and (c == 1).sum() > 100             # case C: empty and one-point bins


@pytest.mark.parametrize("name", make_regrid.CASES)
def test_host_mean_regrid_equals_the_reference_bitwise(gold, name):
    from picaso_amd import justdoit as jdi
    x, y, newx, R = make_regrid.case(name)
    for r in range(make_regrid.NROWS):
        with np.errstate(all="ignore"):
            cx, m = jdi.mean_regrid(x, y[r], newx=newx, R=R)
        assert np.array_equal(cx, gold[name + "/centres"])
        assert np.array_equal(m, gold[name + "/expected"][r], equal_nan=True), (name, r)


def test_plan_errors():
    from picaso_amd import justdoit as jdi
    x = np.linspace(2000.0, 30000.0, 300)
    for kw in ({}, {"newx": np.array([3000.0, 4000.0]), "R": 100}):
        with pytest.raises(Exception, match="Please either enter a newx or a R"):
            jdi.regrid_plan(x, **kw)
        with pytest.raises(Exception, match="Please either enter a newx or a R"):
            jdi.mean_regrid(x, x, **kw)
    for bad in ([3000.0, 3000.0, 4000.0], [3000.0, 5000.0, 4000.0]):
        with pytest.raises(Exception, match="strictly increasing"):
            jdi.regrid_plan(x, newx=np.array(bad))
    with pytest.raises(Exception, match="must be increasing"):
        jdi.regrid_plan(x[::-1], R=100)
    with pytest.raises(Exception, match="must be increasing"):
        jdi.regrid_plan(np.array([1.0, 2.0, 2.0, 3.0]), newx=np.array([1.0, 2.0]))


def test_plan_is_cached_on_the_opacity_object_by_content():
    from picaso_amd import justdoit as jdi

    class Opa:
        pass
    opa = Opa()
    opa.wno = np.linspace(2000.0, 30000.0, 500)
    opa.nwno = 500
    p1 = jdi.regrid_plan(opa, R=50)
    assert jdi.regrid_plan(opa, R=50.0) is p1
    assert jdi.regrid_plan(opa, R=60) is not p1
    nx = np.linspace(3000.0, 20000.0, 30)
    q1 = jdi.regrid_plan(opa, newx=nx)
    assert jdi.regrid_plan(opa, newx=nx.copy()) is q1                  # equal values, another array
    nx[3] = np.nextafter(nx[3], 0.0)                                   # ... and the smallest edit is another plan
    assert jdi.regrid_plan(opa, newx=nx) is not q1
    from picaso_amd import regrid
    assert regrid.resolve({"R": 50}, opa) is p1 and regrid.resolve(p1, opa) is p1
    other = Opa()
    other.wno, other.nwno = np.linspace(2000.0, 30000.0, 400), 400
    with pytest.raises(Exception, match="another wavenumber grid"):
        regrid.resolve(p1, other)
    with pytest.raises(Exception, match="regrid must be"):
        regrid.resolve(100, opa)
