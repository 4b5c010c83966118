"""``picaso_amd.analyze`` on the device (csrc/gridfit.hip) against tests/golden/gridfit.npz -- the reference's own
``custom_interp``, ``mean_regrid``, ``fit_grid`` and likelihood expression on tests/gridfit_cases.py's inputs
(tests/golden/make_gridfit.py).

Bit identity where it is derived: an interpolated spectrum is the reference's products and additions in its order, a binned
model is ``np.bincount``'s chain of additions over columns formed in registers.  Where the order of a sum differs from
numpy's pairwise one (the offset, chi squared, the log likelihood; a decreasing grid's bins) the bound is the rounding
of that many operations, written out at each test.  u = 2^-53."""
import os

import numpy as np
import pytest

import gridfit_cases as gc
from helpers import GOLDEN
from test_gridfit_host import hole_bound

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
COMBOS = [("o1", True, "ndata"), ("o1", True, "nparams"), ("o0", False, "ndata"), ("o0", False, "nparams")]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "gridfit.npz"))


def _fitter(case, prep=True):
    from picaso_amd import analyze
    f = analyze.GridFitter("g", wavelength=case[0], spectra=case[1], grid_params=case[2], verbose=False)
    if prep:
        f.prep_gridtrieval("g")
    return f


@pytest.fixture(scope="module")
def fit():
    """F1's fitter with both data sets, prepared for interpolation (L1 runs on it)."""
    f = _fitter(gc.fit_case())
    for data in ("F1", "F1b"):
        f.add_data(data, *gc.fit_data(data))
    return f


@pytest.fixture(scope="module")
def l1(fit):
    """L1 in one call: ``(logl (200), binned (200, 56))``."""
    from picaso_amd import analyze
    goals, offset, scaling, err_inf = gc.loglike_case()
    return analyze.loglike_batch(goals, fit, "g", "F1b", offset=offset, scaling=scaling, err_inf=err_inf, return_binned=True)


# ------------------------------------------------------------------------------------------------- interpolation
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5])
def test_interp_batch_and_custom_interp_equal_the_reference_bitwise(gold, d):
    from picaso_amd import analyze
    case = gc.interp_case(d)
    f = _fitter(case)
    out = analyze.interp_batch(case[3], f, "g")
    assert out.shape == (gc.NGOALS_I, gc.NWAVE_I)
    assert np.array_equal(out[:, ::gc.PROBE], gold["I%d/probe" % d])
    assert np.array_equal(gc.digest(out), gold["I%d/digest" % d])              # every column, by its bits
    for s in (0, 2, 17):
        assert np.array_equal(analyze.custom_interp(case[3][s], f, "g"), out[s])


def test_missing_node_fallback_within_its_rounding(gold):
    """I6: |got - reference| <= 8 u sum|w_k y_k| / sum(w) -- three rounded products, two additions, the division and the
    weight sum, in any order, with or without FMA in the reference's BLAS dot."""
    from picaso_amd import analyze
    case = gc.hole_case()
    f = _fitter(case)
    out = analyze.interp_batch(case[3], f, "g")
    want = gold["I6/expected"]
    bound = hole_bound(case[1], *analyze.interp_tables(case[3], f, "g"))
    err = np.abs(out[:11] - want[:11])
    print("I6: worst error / bound %.3f" % np.max(err / bound[:11]))
    assert np.all(err <= bound[:11])
    assert np.all(np.isnan(out[11])) and np.all(np.isnan(want[11]))           # exactly on an existing model: dd = 0


# ------------------------------------------------------------------------------------------------- fit_grid
def test_fit_grid_binned_models_equal_mean_regrid_bitwise(gold, fit):
    for data in ("F1", "F1b"):
        fit.fit_grid("g", data, offset=False)
        binned = fit.best_fits["g"][data] - fit.offsets["g"][data][:, None]
        assert np.all(fit.offsets["g"][data] == 0.0)
        assert np.array_equal(binned, gold[data + "/binned"], equal_nan=True), data
    # an empty bin is NaN in every model, so every chi squared is, as in the reference
    assert np.all(np.isnan(fit.chi_sqs["g"]["F1"])) and np.isnan(gold["F1/binned"]).any()


@pytest.mark.parametrize("oname,offset,dof", COMBOS)
def test_fit_grid_offsets_chi_squares_rank_and_posteriors(gold, fit, oname, offset, dof):
    cen, wid, y, e = gc.fit_data("F1b")
    n = y.size
    fit.fit_grid("g", "F1b", dof=dof, offset=offset)
    key = "F1b/%s_%s/" % (oname, dof)
    m = gold["F1b/binned"]
    shift, ref_shift = fit.offsets["g"]["F1b"], gold[key + "shift"]
    if offset:
        # the mean of n terms through a tree and one division: (n + 2) u mean|y - m| of the exact mean; the reference's
        # curve_fit stops at its own distance from it, which (doubled) is the margin of the comparison with the reference
        exact = gold["F1b/shift_exact"]
        b_exact = (n + 2) * U * np.mean(np.abs(y - m), axis=1)
        print("shift: |dev - exact| / bound %.3f, |ref - exact| / |exact| %.2e"
              % (np.max(np.abs(shift - exact) / b_exact), np.max(np.abs(ref_shift - exact) / np.abs(exact))))
        assert np.all(np.abs(shift - exact) <= b_exact)
        assert np.all(np.abs(shift - ref_shift) <= b_exact + 2 * np.abs(ref_shift - exact))
        assert np.array_equal(gold["F1b/shift_margin"], 2 * np.abs(gold["F1b/o1_ndata/shift"] - exact))
    else:
        assert np.all(shift == 0.0)
    assert np.array_equal(fit.best_fits["g"]["F1b"], m + shift[:, None])
    # chi squared is quadratic in the shift: moving the reference's shift by ds changes its sum by exactly
    # -2 ds sum(r / e^2) + ds^2 sum(1 / e^2), r the reference's residual; the rest is the rounding of n + 8 operations
    ndof = n - (0 if dof == "ndata" else 3)
    chi2, ref = fit.chi_sqs["g"]["F1b"], gold[key + "chi2"]
    ds = shift - ref_shift
    r = y - gold[key + "best"]
    bound = (n + 8) * U * ref + np.abs(2 * np.sum(r / e ** 2, axis=1) * ds - ds ** 2 * np.sum(1 / e ** 2)) / ndof
    print("chi2: worst error / bound %.3f (relative error %.2e)" % (np.max(np.abs(chi2 - ref) / bound),
                                                                   np.max(np.abs(chi2 - ref) / ref)))
    assert np.all(np.abs(chi2 - ref) <= bound)
    assert np.array_equal(fit.rank["g"]["F1b"], gold[key + "rank"])
    # a posterior is a sum of exp(-chi2 / 2) over the normaliser: half of chi squared's error, relative
    for name in gc.NAMES[:3]:
        values, prob = fit.posteriors["g"]["F1b"][name]
        want = gold[key + "post_" + name]
        print("posterior %s: worst relative error / bound %.3f" % (name, np.max(np.abs(prob - want) / want) / (np.max(bound) / 2)))
        assert np.all(np.abs(prob - want) <= np.max(bound) / 2 * want)


def test_decreasing_wavelength_grid(gold, fit):
    """F2: the grid is reversed at upload, so a bin's sum runs in the opposite order to F1's: count * u * sum|y| per bin
    (count - 1 additions and the division), and the same rank."""
    wl, spectra, gp = gc.fit_case(decreasing=True)
    f = _fitter((wl, spectra, gp), prep=False)
    cen, wid, y, e = gc.fit_data("F1b")
    f.add_data("F1b", cen, wid, y, e)
    f.fit_grid("g", "F1b", offset=False)
    got, want, counts = f.best_fits["g"]["F1b"], gold["F1b/binned"], gold["F1b/counts"]
    from picaso_amd import justdoit as jdi
    inc = gc.fit_case()
    sum_abs = np.stack([jdi.mean_regrid(inc[0], np.abs(s), newx=cen)[1] for s in inc[1]]) * counts
    bound = counts * U * sum_abs
    print("F2: worst error / bound %.3f" % np.max(np.abs(got - want) / bound))
    assert np.all(np.abs(got - want) <= bound)
    f.fit_grid("g", "F1b")
    assert np.array_equal(f.rank["g"]["F1b"], gold["F1b/o1_ndata/rank"])
    # interpolated spectra come back in the caller's (decreasing) order
    from picaso_amd import analyze
    f.prep_gridtrieval("g")
    fit_goals = gc.loglike_case()[0][:3]
    assert np.array_equal(analyze.interp_batch(fit_goals, f, "g")[:, ::-1], analyze.interp_batch(fit_goals, fit, "g"))


# ------------------------------------------------------------------------------------------------- likelihood
def _loglike_bound(y, e, offset, scaling, err_inf, binned):
    """(n + 8) u sum|terms| of -0.5 sum(terms), terms = the squared residual over sigma and the logarithm."""
    sigma = e[None, :] ** 2 + err_inf[:, None]
    terms = ((y[None, :] + offset[:, None]) * scaling[:, None] - binned) ** 2 / sigma
    return (y.size + 8) * U * 0.5 * np.sum(np.abs(terms) + np.abs(np.log(2 * np.pi * sigma)), axis=1)


def test_loglike_batch_fuses_interpolation_and_binning_bitwise(gold, l1):
    """The binned interpolants are mean_regrid(custom_interp(...)) bit for bit although no interpolated spectrum is ever
    stored; the likelihood is a sum of n terms of a few operations each: (n + 8) u sum|terms|."""
    logl, binned = l1
    assert np.array_equal(binned, gold["L1/binned"])
    goals, offset, scaling, err_inf = gc.loglike_case()
    cen, wid, y, e = gc.fit_data("F1b")
    bound = _loglike_bound(y, e, offset, scaling, err_inf, binned)
    err = np.abs(logl - gold["L1/logl"])
    print("L1: worst error / bound %.3f" % np.max(err / bound))
    assert np.all(err <= bound)


def test_scalar_offset_scaling_err_inf(fit, l1):
    from picaso_amd import analyze
    goals = gc.loglike_case()[0][:5]
    cen, wid, y, e = gc.fit_data("F1b")
    logl = analyze.loglike_batch(goals, fit, "g", "F1b")
    want = -0.5 * np.sum((y - l1[1][:5]) ** 2 / e ** 2 + np.log(2 * np.pi * e ** 2), axis=1)
    assert np.all(np.abs(logl - want) <= _loglike_bound(y, e, np.zeros(5), np.ones(5), np.zeros(5), l1[1][:5]))
    with pytest.raises(Exception, match="scaling must be a scalar or"):
        analyze.loglike_batch(goals, fit, "g", "F1b", scaling=np.ones(3))


def test_a_sample_does_not_depend_on_the_launch_shape(fit, l1):
    from picaso_amd import analyze
    goals, offset, scaling, err_inf = gc.loglike_case()
    full = analyze.interp_batch(goals[:64], fit, "g")
    for size in (1, 7, 64):
        for lo in range(0, gc.NGOALS_L if size > 1 else 3, size):
            hi = min(lo + size, gc.NGOALS_L)
            logl, binned = analyze.loglike_batch(goals[lo:hi], fit, "g", "F1b", offset=offset[lo:hi], scaling=scaling[lo:hi],
                                                 err_inf=err_inf[lo:hi], return_binned=True)
            assert np.array_equal(logl, l1[0][lo:hi]) and np.array_equal(binned, l1[1][lo:hi]), (size, lo)
        assert np.array_equal(analyze.interp_batch(goals[:size], fit, "g"), full[:size])


# ------------------------------------------------------------------------------------------------- argument errors
def test_kernel_argument_errors_launch_nothing(fit):
    from picaso_amd import _lib, analyze
    from picaso_amd._lib import PicasoHipError
    from picaso_amd.device import DeviceArray
    lib, dev = _lib.load(), fit._device("g")
    ctx, grid, n, nw = dev["ctx"], dev["spectra"], dev["nrows"], dev["nwave"]
    plan = fit._plan("g", "F1b")
    one, k1 = np.ones((2, 1)), np.ones(2, dtype=np.int32)
    with pytest.raises(PicasoHipError, match=r"row index 24 outside \[0, 24\)"):
        analyze.grid_rows(ctx, grid, n, nw, np.array([[0], [n]]), one, k1, np.ones(2), plan=plan)
    buf = DeviceArray.zeros((256,), ctx)            # stands for every table: a call that is refused reads none of them
    a = buf.addr
    for kmax in (0, 65):
        with pytest.raises(PicasoHipError, match=r"K must be in \[1, 64\], got %d" % kmax):
            _lib.check(lib.picaso_grid_rows_dev(ctx, n, nw, grid.addr, 2, kmax, a, a, a, a, a, 0, None, None), ctx)
    with pytest.raises(PicasoHipError, match="NULL"):
        _lib.check(lib.picaso_grid_rows_dev(ctx, n, nw, None, 2, 1, a, a, a, a, a, 0, None, None), ctx)
    with pytest.raises(PicasoHipError, match="neither out_full nor out_binned"):
        _lib.check(lib.picaso_grid_rows_dev(ctx, n, nw, grid.addr, 2, 1, a, a, a, a, None, 0, None, None), ctx)
    with pytest.raises(PicasoHipError, match="ndata - numparams must be positive, got 3 - 3"):
        _lib.check(lib.picaso_grid_loglike_dev(ctx, 2, 3, a, a, a, 1, None, None, None, None, 1, 3, a, a, a), ctx)
    with pytest.raises(PicasoHipError, match="NULL"):
        _lib.check(lib.picaso_grid_loglike_dev(ctx, 2, 3, a, a, a, 0, a, a, None, a, 0, 0, None, None, None), ctx)
    with pytest.raises(PicasoHipError, match="mode must be 0"):
        _lib.check(lib.picaso_grid_loglike_dev(ctx, 2, 3, a, a, a, 2, a, a, a, a, 0, 0, a, a, a), ctx)
    assert np.all(buf.to_host() == 0.0)             # nothing was written
    # ... and through the fitter: more parameters than data points
    cen, wid, y, e = gc.fit_data("F1b")
    fit.add_data("three", cen[:3], wid[:3], y[:3], e[:3])
    with pytest.raises(PicasoHipError, match="ndata - numparams must be positive"):
        fit.fit_grid("g", "three", dof="nparams")
