"""``picaso_column_quantiles_dev`` (csrc/quantile.hip) and what stands on it -- ``retrieval.bands``, ``PredictionBand``,
``analyze.bands_batch`` -- against bands_cases' ``np.sort`` restatement of ``mquantiles`` on the same inputs (which
test_bands_host.py holds to scipy's own results in tests/golden/bands.npz).  Everything is compared by value, bit for
bit: the kernel sorts exactly and forms a line with numpy's two products and one addition."""
import ctypes
import os

import numpy as np
import pytest

import bands_cases as bc
import gridfit_cases as gc
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

# every power-of-two padding edge, every change of the tile width (1 024 / 2 048 / 4 096 / 8 192 draws) and of the kernel
# (tiles of 2 048 and 8 192 keys: 128 and 512 draws)
DRAWS = [1, 2, 3, 4, 5, 63, 64, 65, 128, 129, 255, 256, 257, 512, 513, 1000, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193,
         16383, 16384]
COLS = [1, 7, 8, 9, 15, 16, 17, 31, 33, 63, 65, 1003]
Q32 = sorted(set(bc.LEVELS) | set(np.arange(25) / 24.0))[:32]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "bands.npz"))


def _lines(y, k, gamma, cols=None):
    """``column_quantiles`` of the host matrix ``y`` (uploaded as it is)."""
    from picaso_amd import retrieval
    from picaso_amd.device import DeviceArray
    return retrieval.column_quantiles(DeviceArray.from_host(y), k, gamma, cols=cols).to_host()


# ------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("S", DRAWS)
def test_draws_sweep(S):
    from picaso_amd import retrieval
    y = bc.matrix(S, 33, seed=1)
    y[S // 3, 4] = np.nan
    got = retrieval.bands(y)
    assert got.shape == (7, 33)
    assert bc.same(got, bc.bands_numpy(y))


@pytest.mark.parametrize("N", COLS)
def test_columns_sweep(N):
    from picaso_amd import retrieval
    y = bc.matrix(100, N, seed=2)
    assert bc.same(retrieval.bands(y), bc.bands_numpy(y))


def test_many_columns():
    """1 000 draws x 20 003 columns: 1 251 tiles, the last one three columns wide."""
    from picaso_amd import retrieval
    y = bc.matrix(1000, 20003, seed=3)
    assert bc.same(retrieval.bands(y), bc.bands_numpy(y))


# ------------------------------------------------------------------------------------------------- values
def _special(S):
    """Columns that exercise the ordering: ties, a constant, infinities, denormals, signed zeros, NaNs of both signs."""
    y = bc.matrix(S, 16, seed=4)
    h = gc.hash01(S, 11)
    snan = np.array([0x7ff0000000000001, 0xfff8000000000123], dtype=np.uint64).view(np.float64)
    y[:, 0] = np.floor(h * 4.0) - 2.0                                   # ties, mixed signs, zeros
    y[:, 1] = -7.25                                                     # all equal
    y[:, 2] = np.where(h < 0.2, -np.inf, np.where(h > 0.8, np.inf, y[:, 2]))
    y[:, 3] = np.where(h < 0.5, -1.0, 1.0) * np.ldexp(0.5 + h, -1070)   # denormals of both signs
    y[:, 4] = np.where(h < 0.5, -0.0, 0.0)                              # -0.0 next to +0.0
    y[:, 5] = np.where(h < 0.3, -0.0, np.where(h < 0.6, 0.0, np.where(h < 0.8, -5e-324, 5e-324)))
    y[S // 2, 6] = np.nan                                               # one NaN
    y[:, 7] = np.where(h < 0.3, np.nan, np.where(h < 0.5, -np.nan, y[:, 7]))
    y[S // 3, 7], y[S // 4, 7] = snan                                   # a signalling and a negative NaN among them
    y[:, 8] = np.where(h < 0.5, np.nan, -np.nan)                        # only NaNs
    y[:, 9] = np.inf
    y[:, 10] = -np.inf
    y[0, 11], y[S - 1, 11] = np.inf, -np.inf                            # one of each
    y[:, 12] = np.where(h < 0.5, np.inf, np.nan)                        # +inf below NaN
    y[:, 13] = np.where(h < 0.5, -1.7976931348623157e308, 1.7976931348623157e308)
    return y


@pytest.mark.parametrize("S", [2, 37, 600, 2500])
def test_special_values(S):
    from picaso_amd import retrieval
    y = _special(S)
    want = bc.bands_numpy(y, Q32)
    got = retrieval.bands(y, Q32)
    assert bc.same(got, want)
    nan = np.isnan(got)
    assert nan[:, 8].all() and (S == 2 or (nan[:, 6].any() and not nan[:, 6].all()))
    bits = got.view(np.uint64)[nan]
    assert np.all((bits >> np.uint64(51)) & np.uint64(1) == 1), "a NaN came back signalling"


def test_single_draw_returns_the_row_and_quiets_a_nan():
    from picaso_amd import retrieval
    y = _special(2)[:1].copy()
    y[0, 0] = np.array([0x7ff0000000000001], dtype=np.uint64).view(np.float64)[0]
    got = retrieval.bands(y)
    assert bc.same(got, np.repeat(y, 7, axis=0))
    assert np.all(got.view(np.uint64)[:, 0] >> np.uint64(51) & np.uint64(1) == 1)


def test_zero_weight_meets_infinity():
    """No shortcut at gamma = 0 or 1: numpy forms both products, 0 * inf is NaN."""
    S = 50
    y = bc.matrix(S, 5, seed=5)
    y[7, 1], y[9, 2], y[11, 3], y[12, 3] = np.inf, -np.inf, np.inf, -np.inf
    k = np.array([S - 1, 1, S - 1, 1, 20], dtype=np.int32)
    gamma = np.array([0.0, 1.0, 1.0, 0.0, 0.25])
    want = bc.lines_numpy(y, k, gamma)
    assert np.isnan(want[0, 1]) and np.isnan(want[1, 2]) and want[2, 1] == np.inf and want[3, 2] == -np.inf
    assert np.isnan(want[0, 3]) and np.isnan(want[1, 3]) and np.isfinite(want[:, 0]).all()
    assert bc.same(_lines(y, k, gamma), want)


# ------------------------------------------------------------------------------------------------- independence
@pytest.mark.parametrize("S", [100, 3000])
def test_column_subrange_with_a_longer_stride(S):
    """The lines of columns [13, 52) of a 70-column matrix (ld = 70 > ncol = 39, another tiling, another alignment)
    are those columns of the whole matrix's lines, and of the columns uploaded alone."""
    y = bc.matrix(S, 70, seed=6)
    k, gamma = bc.table_numpy(S, bc.LEVELS)
    whole = _lines(y, k, gamma)
    part = _lines(y, k, gamma, cols=(13, 52))
    assert part.shape == (7, 39)
    assert np.array_equal(part.view(np.uint64), whole[:, 13:52].view(np.uint64))
    alone = _lines(np.ascontiguousarray(y[:, 13:52]), k, gamma)
    assert np.array_equal(alone.view(np.uint64), part.view(np.uint64))
    assert bc.same(whole, bc.lines_numpy(y, k, gamma))


def test_lines_do_not_depend_on_the_number_of_levels_and_the_input_stays():
    from picaso_amd import retrieval
    from picaso_amd.device import DeviceArray
    y = _special(300)
    d = DeviceArray.from_host(y)
    few, many, one = retrieval.bands(d, bc.LEVELS), retrieval.bands(d, Q32), retrieval.bands(d, [0.5])
    for i, q in enumerate(bc.LEVELS):
        assert np.array_equal(few[i].view(np.uint64), many[Q32.index(q)].view(np.uint64))
    assert np.array_equal(one[0].view(np.uint64), few[6].view(np.uint64))
    assert np.array_equal(d.to_host().view(np.uint64), y.view(np.uint64))


# ------------------------------------------------------------------------------------------------- API
def test_bands_of_host_and_device_arrays_agree():
    from picaso_amd import retrieval
    from picaso_amd.device import DeviceArray
    y = bc.matrix(257, 45, seed=7)
    a, b = retrieval.bands(y), retrieval.bands(DeviceArray.from_host(y))
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and bc.same(a, bc.bands_numpy(y))
    assert bc.same(retrieval.bands(y.tolist(), {"lo": 0.1, "hi": 0.9}), bc.bands_numpy(y, [0.1, 0.9]))


@pytest.mark.parametrize("S", bc.FIXTURE_DRAWS)
def test_prediction_band_equals_mquantiles(gold, S):
    from picaso_amd import retrieval
    y = bc.fixture_matrix(S)
    band = retrieval.PredictionBand(np.arange(bc.FIXTURE_COLS))
    for row in y:
        band.add(row)
    want = gold["M%d/bands" % S]
    assert bc.same(band.get_line(), want[6])
    resident = band._dev
    for i, q in enumerate(bc.LEVELS):
        assert bc.same(band.get_line(q), want[i])
    assert bc.same(band.lines(bc.LEVELS), want)
    assert band._dev is resident, "the matrix was uploaded again"
    if S == 7:
        band.add(y[0])
        assert bc.same(band.get_line(0.5), bc.bands_numpy(np.vstack([y, y[:1]]), [0.5])[0])
        assert band._dev is not resident


@pytest.mark.parametrize("name", ["newx", "none"])
def test_get_evaluations_on_the_device_equals_the_reference(gold, name):
    """The whole function with its two launches against the reference's own results (tests/golden/make_bands.py)."""
    from picaso_amd import retrieval
    samples = bc.toy_samples()
    np.random.seed(bc.SEED_E)
    ev = retrieval.get_evaluations(samples, samples[17], bc.toy_model(), bc.NDRAWS_E, regrid=bc.toy_regrids()[name])
    key = "E/%s/" % name
    assert bc.same(np.stack([ev["bands_spectra"][k] for k in bc.KEYS]), gold[key + "spectra"])
    got = np.stack([[ev["bands_ptchem"][n][k] for k in bc.KEYS] for n in ("temperature", "H2O", "CO2")])
    assert np.array_equal(got, gold[key + "ptchem"])
    assert bc.same(np.asarray(ev["max_logl_spectra"]), gold[key + "max_logl_spectra"])
    chi = retrieval.get_chisq_max(ev, bc.toy_data())
    assert chi["chisq_per_datapt"] == gold[key + "chisq_chisq_per_datapt"]


def _fitter(case):
    from picaso_amd import analyze
    f = analyze.GridFitter("g", wavelength=case[0], spectra=case[1], grid_params=case[2], verbose=False)
    f.prep_gridtrieval("g")
    return f


@pytest.mark.parametrize("d", [2, 4])
def test_bands_batch_equals_bands_of_interp_batch(d):
    from picaso_amd import analyze, retrieval
    case = gc.interp_case(d)
    f = _fitter(case)
    stack = analyze.interp_batch(case[3], f, "g")
    want = retrieval.bands(stack)
    got = analyze.bands_batch(case[3], f, "g")
    assert got.shape == (7, gc.NWAVE_I)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) and bc.same(got, bc.bands_numpy(stack))
    got = analyze.bands_batch(case[3], f, "g", q=[0.25, 0.5])
    assert bc.same(got, bc.bands_numpy(stack, [0.25, 0.5]))


@pytest.mark.parametrize("decreasing", [False, True])
def test_bands_batch_on_a_fit_grid_and_binned_to_data(decreasing):
    """F1 / F2 (the wavelength array decreasing) with L1's 200 goals: in full, in the caller's column order, and binned
    to a data set -- one with empty bins (NaN columns) and one without."""
    from picaso_amd import analyze, retrieval
    f = _fitter(gc.fit_case(decreasing=decreasing))
    goals = gc.loglike_case()[0]
    stack = analyze.interp_batch(goals, f, "g")
    got = analyze.bands_batch(goals, f, "g")
    assert got.shape == (7, gc.NWAVE_F) and bc.same(got, bc.bands_numpy(stack))
    assert np.array_equal(got.view(np.uint64), retrieval.bands(stack).view(np.uint64))
    for data in ("F1", "F1b"):
        f.add_data(data, *gc.fit_data(data))
        binned = analyze.loglike_batch(goals, f, "g", data, return_binned=True)[1]
        got = analyze.bands_batch(goals, f, "g", data_name=data)
        assert got.shape == (7, binned.shape[1])
        assert np.array_equal(got.view(np.uint64), retrieval.bands(binned).view(np.uint64))
        assert bc.same(got, bc.bands_numpy(binned))
        assert np.isnan(got).any() == (data == "F1")


# ------------------------------------------------------------------------------------------------- ABI
def test_bad_arguments_are_errors_and_launch_nothing():
    from picaso_amd import _lib, device
    from picaso_amd.device import DeviceArray
    lib, ctx = _lib.load(), _lib.context()
    S, N = 6, 5
    y = bc.matrix(S, N, seed=8)
    d_y, d_out = DeviceArray.from_host(y, ctx), DeviceArray.from_host(np.full((2, N), 123.0), ctx)
    k, g = (ctypes.c_int * 2)(2, 5), (ctypes.c_double * 2)(0.25, 1.0)
    many_k, many_g = (ctypes.c_int * 33)(*([1] * 33)), (ctypes.c_double * 33)(*([0.5] * 33))
    nan = float("nan")

    def call(nsamp=S, ncol=N, yy=d_y.addr, ld=N, nq=2, kk=k, gg=g, out=d_out.addr, c=ctx):
        return lib.picaso_column_quantiles_dev(c, nsamp, ncol, yy, ld, nq, kk, gg, out)
    bad = {
        "nsamp 0": dict(nsamp=0), "nsamp -1": dict(nsamp=-1), "nsamp above the cap": dict(nsamp=16385),
        "ncol 0": dict(ncol=0), "ncol -3": dict(ncol=-3), "ld < ncol": dict(ld=N - 1),
        "nq 0": dict(nq=0), "nq 33": dict(nq=33, kk=many_k, gg=many_g),
        "k 0": dict(kk=(ctypes.c_int * 2)(0, 5)), "k nsamp": dict(kk=(ctypes.c_int * 2)(2, S)),
        "k negative": dict(kk=(ctypes.c_int * 2)(-4, 1)),
        "gamma < 0": dict(gg=(ctypes.c_double * 2)(-1e-300, 1.0)), "gamma > 1": dict(gg=(ctypes.c_double * 2)(0.5, 1.0000000000000002)),
        "gamma NaN": dict(gg=(ctypes.c_double * 2)(nan, 0.5)),
        "y NULL": dict(yy=None), "k NULL": dict(kk=None), "gamma NULL": dict(gg=None), "out NULL": dict(out=None),
    }
    for what, kw in bad.items():
        assert call(**kw) != 0, what
        msg = lib.picaso_last_error(ctx).decode()
        assert msg.startswith("picaso_column_quantiles_dev: "), (what, msg)
    assert "16384" in (call(nsamp=16385), lib.picaso_last_error(ctx).decode())[1]
    assert call(c=None) != 0 and b"null context" in lib.picaso_last_error(None)
    # a single draw has no table: its k is not looked at, its gamma is
    assert call(nsamp=1, gg=(ctypes.c_double * 2)(2.0, 0.0)) != 0
    device.sync(ctx)
    assert np.all(d_out.to_host() == 123.0), "a refused call wrote its output"
    assert call() == 0
    assert bc.same(d_out.to_host(), bc.lines_numpy(y, [2, 5], [0.25, 1.0]))
    assert call(nsamp=1, kk=(ctypes.c_int * 2)(0, 99)) == 0
    assert bc.same(d_out.to_host(), np.repeat(y[:1], 2, axis=0))
    with pytest.raises(_lib.PicasoHipError, match="PICASO_BANDS_MAX_DRAWS"):
        from picaso_amd import retrieval
        retrieval.column_quantiles(DeviceArray((16385, 1), ctx), [1], [0.5])
