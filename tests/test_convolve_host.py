"""``jdi.convolve_plan`` and ``jdi.conv_non_uniform_R`` (picaso_amd/convolve.py) against tests/golden/convolve.npz -- arrays
the reference's own ``conv_non_uniform_R`` produced (tests/golden/make_convolve.py; reference driver.py:338-381).

The plan cuts every point's sums to the columns within 39 sigma.  That changes nothing only if every weight the reference
forms outside the window is an exact 0.0, which is checked here column by column.  The tolerance is derived, not measured:
with the argument of ``exp`` bit-equal, a windowed evaluation differs from the reference by the rounding of ``exp`` (1 ulp
on either side) and the order of two sums of ``n_w`` non-negative terms (``(n_w - 1) 2^-53`` each), hence
``|out - ref| <= (2 n_w + 10) 2^-53 conv(|y|)`` with ``n_w`` the point's own count.  No GPU: a plan uploads nothing until a
spectrum uses it."""
import importlib.util
import os

import numpy as np
import pytest

from helpers import GOLDEN

_spec = importlib.util.spec_from_file_location("make_convolve", os.path.join(GOLDEN, "make_convolve.py"))
make_convolve = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_convolve)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "convolve.npz"))


def bound(counts, conv_abs):
    """the derived tolerance per point: ``(2 n_w + 10) 2^-53 conv(|y|)``"""
    return (2.0 * np.asarray(counts) + 10.0) * 2.0 ** -53 * np.asarray(conv_abs)


def within(got, ref, counts, conv_abs):
    """NaN where and only where the reference has it, and every other point inside the bound; returns the worst ratio"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    err, lim = np.abs(got[ok] - ref[ok]), np.broadcast_to(bound(counts, conv_abs), ref.shape)[ok]
    assert np.all(err <= lim), float(np.max(err / np.where(lim > 0, lim, 1.0)))
    return float(np.max(err / lim)) if err.size else 0.0


@pytest.mark.parametrize("name", make_convolve.CASES)
def test_fixture_inputs_are_rebuilt_bit_for_bit(gold, name):
    x, y, wl, R = make_convolve.case(name)
    assert y.shape == (2, x.size)
    assert np.array_equal(y[:, ::97], gold[name + "/y_probe"])
    assert np.array_equal(wl, gold[name + "/wl"]) and np.array_equal(R, gold[name + "/R"])
    assert np.array_equal(gold[name + "/expected"][0], gold[name + "/expected_abs"][0], equal_nan=True)      # the positive row


@pytest.mark.parametrize("name", make_convolve.CASES)
def test_every_reference_weight_outside_the_window_is_zero(name):
    from picaso_amd import justdoit as jdi
    x, y, wl, R = make_convolve.case(name)
    plan = jdi.convolve_plan(x, wl, R)
    assert plan.nobs == wl.size and plan.nwno == x.size
    assert plan.lo.dtype == np.int32 and plan.hi.dtype == np.int32
    assert np.all(plan.lo >= 0) and np.all(plan.hi <= x.size) and np.all(plan.lo <= plan.hi)
    assert np.array_equal(plan.counts, plan.hi - plan.lo)
    assert np.array_equal(plan.model_wl, 1e4 / x) and np.array_equal(plan.out_wavenumber, 1e4 / wl)
    model_wl = 1e4 / x
    for i in range(plan.nobs):
        sigma = wl[i] / R[i] / 2.355
        weight = np.exp(-((model_wl - wl[i]) ** 2) / (2 * sigma ** 2))          # the reference's weights of point i
        assert plan.den[i] == 2 * sigma ** 2
        inside = np.zeros(x.size, dtype=bool)
        inside[plan.lo[i]:plan.hi[i]] = True
        assert np.all(weight[~inside] == 0.0), (name, i)
        assert np.all(np.abs(model_wl[inside] - wl[i]) <= 39.0 * sigma * (1 + 1e-12))
        assert np.all(np.abs(model_wl[~inside] - wl[i]) >= 39.0 * sigma * (1 - 1e-12))


def test_edge_cases_are_what_the_issue_says():
    from picaso_amd import justdoit as jdi
    plan = {n: jdi.convolve_plan(*[make_convolve.case(n)[k] for k in (0, 2, 3)]) for n in make_convolve.CASES}
    assert 1100 <= plan["A"].counts.max() <= 1200
    assert plan["B"].counts.max() < 1024 and plan["B"].counts.min() < 64
    assert plan["C"].counts.max() > 4096 // 2
    wl = make_convolve.case("C")[2]
    assert np.all(np.diff(wl[:7]) < 0) and wl[7] == wl[3]
    assert list(plan["D"].counts > 0) == [False, True, True, True, False]
    assert list(plan["E"].counts) == [0, 1, 2, 63, 64, 65]


@pytest.mark.parametrize("name", make_convolve.CASES)
def test_host_conv_non_uniform_R_against_the_reference(gold, name):
    from picaso_amd import justdoit as jdi
    x, y, wl, R = make_convolve.case(name)
    counts = jdi.convolve_plan(x, wl, R).counts
    for r in range(2):
        got = jdi.conv_non_uniform_R(y[r], 1e4 / x, R, wl)
        within(got, gold[name + "/expected"][r], counts, gold[name + "/expected_abs"][r])
    if name == "D":
        assert list(np.isnan(gold["D/expected"][0])) == [True, False, False, False, True]


def test_scalar_R_is_every_points_R():
    from picaso_amd import justdoit as jdi
    x, y, wl, _ = make_convolve.case("A")
    assert np.array_equal(jdi.conv_non_uniform_R(y[0], 1e4 / x, 80, wl), jdi.conv_non_uniform_R(y[0], 1e4 / x, np.full(37, 80.0), wl))
    assert np.array_equal(jdi.convolve_plan(x, wl, 80).den, jdi.convolve_plan(x, wl, np.full(37, 80.0)).den)


class _Opa:
    def __init__(self, n):
        self.wno, self.nwno = np.linspace(2000.0, 30000.0, n), n


def test_plan_is_cached_on_the_opacity_object_by_content():
    from picaso_amd import convolve
    from picaso_amd import justdoit as jdi
    opa = _Opa(500)
    wl = np.linspace(0.5, 4.0, 20)
    p1 = jdi.convolve_plan(opa, wl, 100)
    assert isinstance(p1, jdi.ConvolvePlan)
    assert jdi.convolve_plan(opa, wl.copy(), 100.0) is p1
    assert jdi.convolve_plan(opa, wl, 120) is not p1
    q1 = jdi.convolve_plan(opa, wl, np.linspace(30, 300, 20))
    assert jdi.convolve_plan(opa, list(wl), np.linspace(30, 300, 20)) is q1
    wl2 = wl.copy()
    wl2[3] = np.nextafter(wl2[3], 0.0)                                  # the smallest edit is another plan
    assert jdi.convolve_plan(opa, wl2, 100) is not p1
    assert convolve.resolve({"wl": wl, "R": 100}, opa) is p1 and convolve.resolve(p1, opa) is p1
    assert convolve.reduction(None, {"wl": wl, "R": 100}, opa) is p1 and convolve.reduction(None, None, opa) is None
    assert convolve.reduction({"R": 50}, None, opa) is jdi.regrid_plan(opa, R=50)
    assert p1._dev == {}                                                # nothing is uploaded before a spectrum uses it


def test_errors():
    from picaso_amd import convolve
    from picaso_amd import justdoit as jdi
    opa = _Opa(500)
    wl = np.linspace(0.5, 4.0, 20)
    for R in (0, -5.0, np.where(np.arange(20) == 4, 0.0, 100.0), np.nan):
        with pytest.raises(Exception, match="R must be positive"):
            jdi.convolve_plan(opa, wl, R)
    for R in (np.full(19, 100.0), np.full((20, 1), 100.0), [100.0, 100.0]):
        with pytest.raises(Exception, match="different lengths"):
            jdi.convolve_plan(opa, wl, R)
    with pytest.raises(Exception, match="positive and finite"):
        jdi.convolve_plan(opa, np.array([1.0, -2.0]), 100)
    with pytest.raises(Exception, match="non-empty 1-D"):
        jdi.convolve_plan(opa, np.array([]), 100)
    with pytest.raises(Exception, match="strictly monotone"):
        jdi.convolve_plan(np.array([1.0, 2.0, 2.0, 3.0]), wl, 100)
    plan = jdi.convolve_plan(opa, wl, 100)
    with pytest.raises(Exception, match="another wavenumber grid"):
        convolve.resolve(plan, _Opa(400))
    with pytest.raises(Exception, match="convolve must be"):
        convolve.resolve(100, opa)
    with pytest.raises(Exception, match="convolve must be"):
        convolve.resolve({"wl": wl}, opa)
    with pytest.raises(Exception, match="give one of them"):
        convolve.reduction({"R": 50}, {"wl": wl, "R": 100}, opa)


def test_public_calls_refuse_before_anything_runs():
    """the combinations that are errors raise before the opacity object or the case is touched: no GPU is needed"""
    from picaso_amd import justdoit as jdi
    opa = _Opa(500)
    wl = np.linspace(0.5, 4.0, 20)
    spec = {"wl": wl, "R": 100}
    case = jdi.inputs()
    with pytest.raises(Exception, match="give one of them"):
        jdi.picaso(case, opa, regrid={"R": 50}, convolve=spec)
    with pytest.raises(Exception, match="give one of them"):
        jdi.picaso_async(case, opa, regrid={"R": 50}, convolve=spec)
    with pytest.raises(Exception, match="give one of them"):
        jdi.spectrum_batch([case], opa, regrid={"R": 50}, convolve=spec)
    with pytest.raises(NotImplementedError, match="convolve= with devices=N"):
        jdi.picaso(case, opa, devices=2, convolve=spec)
    with pytest.raises(NotImplementedError, match="phase_curve"):
        case.phase_curve(opa, convolve=spec)
    with pytest.raises(Exception, match="another wavenumber grid"):
        jdi.picaso(case, opa, convolve=jdi.convolve_plan(_Opa(400), wl, 100))
    with pytest.raises(Exception, match="R must be positive"):
        jdi.picaso(case, opa, convolve={"wl": wl, "R": -1})
    with pytest.raises(Exception, match="different lengths"):
        jdi.picaso(case, opa, convolve={"wl": wl, "R": np.full(3, 100.0)})
    assert jdi.picaso(case, opa, calculation="nothing", convolve=spec).keys() == {"wavenumber", "convolve_counts"}


def test_the_symbol_is_declared_in_the_header():
    with open(os.path.join(ROOT, "include", "picaso_hip.h")) as fh:
        text = fh.read()
    assert "int picaso_lsf_convolve_dev(picaso_ctx *ctx, long nwno, const double *wl, int nobs" in text
    assert "driver.py:338-381" in text
