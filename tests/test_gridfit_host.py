"""``picaso_amd.analyze`` on the host: the tables ``interp_tables`` builds for ``picaso_grid_rows_dev``, the reference's
host functions, and the error paths.  Fixture: tests/golden/gridfit.npz, the reference's own ``custom_interp`` /
``fit_grid`` / ``get_chi_posteriors`` output on tests/gridfit_cases.py's inputs (tests/golden/make_gridfit.py).

The kernel's formula is restated in numpy (``gridfit_cases.eval_tables``: per sample ``(((0.0 + w0 g[r0]) + w1 g[r1]) +
...) / div``, each operation rounded); the tables pushed through it must be the reference's ``custom_interp`` bit for bit --
the claim the device path rests on, checked here without a device.  Nothing is uploaded: a fitter's spectra go to the
device when a device path first reads them."""
import os

import numpy as np
import pytest

import gridfit_cases as gc
from helpers import GOLDEN

U = 2.0 ** -53


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "gridfit.npz"))


def _fitter(case, prep=True):
    from picaso_amd import analyze
    f = analyze.GridFitter("g", wavelength=case[0], spectra=case[1], grid_params=case[2], verbose=False)
    if prep:
        f.prep_gridtrieval("g")
    return f


def test_fixture_inputs_are_rebuilt_bit_for_bit(gold):
    for d in range(1, 6):
        wl, spectra, gp, goals = gc.interp_case(d)
        assert np.array_equal(np.concatenate([spectra[:, ::97].ravel(), goals.ravel()]), gold["I%d/in_probe" % d])
    wl, spectra, gp, goals = gc.hole_case()
    assert np.array_equal(np.concatenate([spectra[:, ::97].ravel(), goals.ravel()]), gold["I6/in_probe"])
    wl, spectra, gp = gc.fit_case()
    for data in ("F1", "F1b"):
        cen, wid, y, e = gc.fit_data(data)
        assert np.array_equal(np.concatenate([spectra[:, ::97].ravel(), cen, y, e]), gold[data + "/in_probe"])
    goals, offset, scaling, err_inf = gc.loglike_case()
    assert np.array_equal(np.concatenate([goals.ravel(), offset, scaling, err_inf]), gold["L1/in_probe"])


@pytest.mark.parametrize("d", [1, 2, 3, 4, 5])
def test_tables_through_the_kernel_formula_are_custom_interp_bitwise(gold, d):
    from picaso_amd import analyze
    case = gc.interp_case(d)
    f = _fitter(case)
    rows, wts, kcount, div = analyze.interp_tables(case[3], f, "g")
    assert rows.shape == wts.shape == (gc.NGOALS_I, 2 ** d) and rows.dtype == np.int32
    assert np.all(kcount == 2 ** d) and np.all(div == 1.0) and rows.min() >= 0 and rows.max() < case[1].shape[0]
    out = gc.eval_tables(case[1], rows, wts, kcount, div)
    assert np.array_equal(out[:, ::gc.PROBE], gold["I%d/probe" % d])
    assert np.array_equal(gc.digest(out), gold["I%d/digest" % d])


def test_goal_on_a_node_returns_that_model(gold):
    """Goal 1 of every case sits on the first node of every parameter: all weight on one corner."""
    from picaso_amd import analyze
    case = gc.interp_case(3)
    f = _fitter(case)
    rows, wts, kcount, div = analyze.interp_tables(case[3][1:2], f, "g")
    assert wts[0, 0] == 1.0 and np.all(wts[0, 1:] == 0.0)
    cols = np.stack([case[2]["planet_params"][n] for n in gc.NAMES[:3]], axis=1)
    assert np.array_equal(cols[rows[0, 0]], case[3][1])


def hole_bound(spectra, rows, wts, kcount, div):
    """8 * 2^-53 * sum|w_k y_k| / sum(w) per sample and column."""
    with np.errstate(all="ignore"):                  # a sample on an existing model: inf weights, NaN
        return np.stack([8 * U * np.sum(np.abs(wts[s, :3, None] * spectra[rows[s, :3]]), axis=0) / div[s]
                         for s in range(rows.shape[0])])


def test_missing_node_takes_the_three_neighbour_fallback(gold):
    from picaso_amd import analyze
    case = gc.hole_case()
    f = _fitter(case)
    assert f.interp_params["g"]["node_rows"][1, 1] == -1 and np.sum(f.interp_params["g"]["node_rows"] < 0) == 1
    rows, wts, kcount, div = analyze.interp_tables(case[3], f, "g")
    assert rows.shape == (12, 4) and np.all(kcount == 3)
    assert np.array_equal(div, np.array([np.sum(w[:3]) for w in wts]))
    out = gc.eval_tables(case[1], rows, wts, kcount, div)
    want = gold["I6/expected"]
    assert np.all(np.isnan(out[11])) and np.all(np.isnan(want[11]))           # exactly on an existing model: dd = 0
    assert np.all(np.abs(out[:11] - want[:11]) <= hole_bound(case[1], rows, wts, kcount, div)[:11])


def test_square_grid_is_built_when_read():
    case = gc.hole_case()
    f = _fitter(case)
    ip = f.interp_params["g"]
    assert "square_spectra_grid" not in ip
    sq = ip["square_spectra_grid"]
    assert sq.shape == (3, 3, case[1].shape[1]) and np.all(np.isnan(sq[1, 1])) and np.sum(np.isnan(sq[..., 0])) == 1
    rows = ip["node_rows"]
    assert np.array_equal(sq[0, 2], case[1][rows[0, 2]])
    assert list(ip["grid_parameters_unique"]) == ["mh", "cto"]
    assert ip["offset_prior"] == abs(2 * (np.min(case[1]) - np.max(case[1])))


def test_duplicate_models_and_nan_rows():
    from picaso_amd import analyze
    wl, spectra, gp, goals = gc.interp_case(2)
    n = spectra.shape[0]
    spectra2 = np.concatenate([spectra, spectra[:1] * 2.0])                   # a second model on model 0's node
    gp2 = {k: {kk: np.concatenate([vv, vv[:1]]) for kk, vv in v.items()} for k, v in gp.items()}
    f = _fitter((wl, spectra2, gp2))
    assert n not in f.interp_params["g"]["node_rows"]                        # the first match counts
    spectra3 = spectra.copy()
    spectra3[5, 77] = np.nan
    f = _fitter((wl, spectra3, gp))
    assert np.sum(f.interp_params["g"]["node_rows"] < 0) == 1 and 5 not in f.interp_params["g"]["node_rows"]
    rows, wts, kcount, div = analyze.interp_tables(goals, f, "g")
    assert set(kcount.tolist()) == {3, 4} and not np.any(rows[np.arange(4)[None, :] < kcount[:, None]] == 5)


def test_host_functions_are_the_references():
    from picaso_amd import analyze
    arr = np.array([1.0, 2.0, 4.0])
    assert analyze.find_bounding_values(arr, 2.5) == ([2.0, 4.0], [1, 2])
    assert analyze.find_bounding_values(arr, 4.0) == ([2.0, 4.0], [1, 2])
    assert analyze.find_bounding_values(arr, 9.0) == ([2.0, 4.0], [1, 2])
    assert analyze.find_bounding_values(arr, 1.0) == ([1.0, 2.0], [0, 1])
    assert analyze.find_bounding_values(arr, 0.5) == [1.0]
    a = np.arange(24.0).reshape(2, 3, 4)
    assert np.array_equal(analyze.get_last_dimension(a, [1, 2, -1]), a[1, 2])
    assert np.array_equal(analyze.get_last_dimension(a, [-1]), a)
    y, e, m = np.array([1.0, 2.0, 3.5]), np.array([0.1, 0.2, 0.3]), np.array([1.1, 1.7, 3.0])
    assert analyze.chi_squared(y, e, m, 1) == np.sum(((y - m) / e) ** 2) / 2


def test_custom_array_is_interpolated_on_the_host(gold):
    """``to_interp='custom'`` with the square spectra grid itself: the reference's loop, so the spectrum's bits."""
    from picaso_amd import analyze
    case = gc.interp_case(2)
    f = _fitter(case)
    sq = f.interp_params["g"]["square_spectra_grid"]
    out = np.stack([analyze.custom_interp(g, f, "g", to_interp="custom", array_to_interp=sq) for g in case[3][:6]])
    assert np.array_equal(out[:, ::gc.PROBE], gold["I2/probe"][:6])
    temp = np.arange(3 * 4 * 5, dtype=float).reshape(3, 4, 5)
    on_node = analyze.custom_interp(case[3][1], f, "g", to_interp="custom", array_to_interp=temp)
    assert np.array_equal(on_node, temp[0, 0])


@pytest.mark.parametrize("combo", ["o1_ndata", "o1_nparams", "o0_ndata", "o0_nparams"])
def test_chi_posteriors_from_the_golden_chi_squares(gold, combo):
    case = gc.fit_case()
    f = _fitter(case, prep=False)
    f.chi_sqs = {"g": {"F1b": gold["F1b/%s/chi2" % combo]}}
    for name in gc.NAMES[:3]:
        values, prob = f.get_chi_posteriors("g", "F1b", name)
        assert np.array_equal(values, np.unique(case[2]["planet_params"][name]))
        assert np.array_equal(prob, gold["F1b/%s/post_%s" % (combo, name)])
    with pytest.raises(Exception, match="not found in grid"):
        f.get_chi_posteriors("g", "F1b", "logg")


def test_add_grid_bookkeeping():
    case = gc.interp_case(5)
    f = _fitter(case, prep=False)
    n = case[1].shape[0]
    assert f.grids == ["g"] and f.list_of_files["g"] == list(range(n)) and f.save_chem is False
    assert f.overview["g"]["num_params"] == 5 and f.wavelength["g"] is not None and f.spectra["g"].shape == (n, gc.NWAVE_I)
    assert list(f.grid_params["g"]) == ["planet_params", "cld_params"]
    assert np.array_equal(f.overview["g"]["cld_params"]["fsed"], np.array(gc.NODE_VALUES[4][:3]))
    f.add_data("d", np.array([1.0, 2.0]), np.array([1.0, 1.0]), np.array([0.1, 0.2]), np.array([0.01, 0.01]))
    assert set(f.data["d"]) == {"wlgrid_center", "wlgrid_width", "y_data", "e_data"}


def test_error_paths():
    from picaso_amd import analyze
    wl, spectra, gp, goals = gc.interp_case(2)
    f = _fitter((wl, spectra, gp))
    with pytest.raises(Exception, match=r"mh = -1\.5 is below the grid.*\[-1\.0, 0\.5\]"):
        analyze.interp_tables(np.array([[-1.5, 0.3]]), f, "g")
    with pytest.raises(Exception, match=r"cto = .*below the grid.*\[0\.25, 0\.916\]"):
        analyze.interp_tables(np.array([[0.0, 0.3], [0.0, 0.2]]), f, "g")
    with pytest.raises(Exception, match="one value per grid parameter"):
        analyze.interp_tables(np.array([[0.0, 0.3, 1.0]]), f, "g")
    # a parameter with a single value
    one = {"planet_params": dict(gp["planet_params"], tint=np.full(spectra.shape[0], 100.0))}
    f1 = _fitter((wl, spectra, one))
    assert f1.overview["g"]["num_params"] == 2 and f1.overview["g"]["planet_params"]["tint"] == 100.0
    with pytest.raises(Exception, match="tint has the single value 100.0"):
        analyze.interp_tables(np.array([[0.0, 0.3, 100.0]]), f1, "g")
    # d > 6
    cols = np.array([[(m >> p) & 1 for p in range(7)] for m in range(128)], dtype=float)
    seven = {"planet_params": {"p%d" % p: cols[:, p] for p in range(7)}}
    f7 = _fitter((np.array([1.0, 2.0, 3.0]), np.ones((128, 3)), seven))
    with pytest.raises(Exception, match="7 parameters.*at most 6"):
        analyze.interp_tables(np.full((1, 7), 0.5), f7, "g")
    # inf in the spectra, a wavelength grid that turns, shapes
    bad = spectra.copy()
    bad[3, 100] = -np.inf
    with pytest.raises(Exception, match="inf"):
        _fitter((wl, bad, gp), prep=False)
    turn = wl.copy()
    turn[10] = turn[9]
    with pytest.raises(Exception, match="strictly monotonic"):
        _fitter((turn, spectra, gp), prep=False)
    with pytest.raises(Exception, match="spectra must be"):
        _fitter((wl[:-1], spectra, gp), prep=False)
    with pytest.raises(NotImplementedError, match="add_grid"):
        analyze.GridFitter("g", model_dir="/some/where")
    with pytest.raises(Exception, match="not prepared"):
        analyze.interp_tables(goals, _fitter((wl, spectra, gp), prep=False), "g")
    with pytest.raises(Exception, match="Parameter logg not found in grid g"):
        f.chi_sqs = {"g": {"d": np.ones(spectra.shape[0])}}
        f.get_chi_posteriors("g", "d", "logg")


def test_table_checks_come_before_any_upload():
    """``grid_rows`` refuses a broken table before it touches the device (so this runs without one)."""
    from picaso_amd import analyze
    from picaso_amd._lib import PicasoHipError
    one, k1 = np.ones((2, 1)), np.ones(2, dtype=np.int32)
    with pytest.raises(PicasoHipError, match=r"row index 5 outside \[0, 5\)"):
        analyze.grid_rows(None, None, 5, 10, np.array([[0], [5]]), one, k1, np.ones(2), full=True)
    with pytest.raises(PicasoHipError, match="row index -1"):
        analyze.grid_rows(None, None, 5, 10, np.array([[-1], [0]]), one, k1, np.ones(2), full=True)
    with pytest.raises(PicasoHipError, match=r"K must be in \[1, 64\], got 65"):
        analyze.grid_rows(None, None, 5, 10, np.zeros((2, 65), dtype=np.int32), np.ones((2, 65)), k1, np.ones(2), full=True)
    with pytest.raises(PicasoHipError, match=r"K must be in \[1, 64\], got 0"):
        analyze.grid_rows(None, None, 5, 10, np.zeros((2, 0), dtype=np.int32), np.ones((2, 0)), k1, np.ones(2), full=True)
    with pytest.raises(PicasoHipError, match="count is outside"):
        analyze.grid_rows(None, None, 5, 10, np.zeros((2, 1), dtype=np.int32), one, np.array([1, 0]), np.ones(2), full=True)


def test_gridfit_kernels_compile_for_gfx950_without_spills():
    """hipcc's own resource report for csrc/gridfit.hip: no scratch and no spilled register in any of its kernels."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import resource_usage
    rows = {r["name"]: r for r in resource_usage.table(os.path.join(root, "picaso_amd", "csrc", "gridfit.hip"))}
    kernels = [n for n in rows if "k_grid_" in n]
    assert len(kernels) == 3, sorted(rows)
    for n in kernels:
        r = rows[n]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
        assert r["VGPRs"] <= 64 and r["LDS Size"] <= 2048, r
