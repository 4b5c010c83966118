"""What jdi.photon_attenuation / taumap / heatmap_taus / cloud_optics_1d need without a GPU: the fixture
(tests/golden/attenuation.npz, written by tests/golden/make_attenuation.py), the C entry points, and the host tables --
the bins of ``R``, the wavelength window and the wavelength index."""
import os

import numpy as np
import pytest

from helpers import GOLDEN

NEW = ("picaso_tau_level_dev", "picaso_band_mean_rows_dev")
SCENES = {"s13": (13, 1), "s3": (3, 1), "s2": (2, 1), "ck13": (13, 3)}


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLDEN, "attenuation.npz"))


def test_fixture_loads_and_holds_the_deliberate_columns(fix):
    assert list(fix["scenes"]) == list(SCENES) and list(fix["at_taus"]) == [0.0, 0.5, 1.0, 1e6]
    col = dict(zip((str(n) for n in fix["col_names"]), (int(c) for c in fix["cols"])))
    assert set(col) == {"zero_cloud", "opaque", "top_zeros", "ties", "thin", "nan"}
    assert {c // 64 for c in col.values()} == {0, 1, 2}                       # every 64-lane tile has some
    for name, (nlevel, ngauss) in SCENES.items():
        t, nlayer = name + "/", nlevel - 1
        wno = fix[t + "wno"]
        assert wno.size == 150 and np.all(np.diff(wno) > 0)
        for k in ("taugas", "taucld", "tauray"):
            assert fix[t + k].shape == (nlayer, 150, ngauss), k
            assert not (fix[t + k] < 0).any()
        assert fix[t + "cloud/w0"].shape == (nlayer, 150) and fix[t + "level/pressure"].shape == (nlevel,)
        gas, cld, ray = fix[t + "taugas"], fix[t + "taucld"], fix[t + "tauray"]
        assert np.all(cld[:, col["zero_cloud"]] == 0) and np.any(cld > 0)
        assert np.nanmax(gas[:, col["opaque"]]) >= 1e4
        if nlayer > 1:
            assert all(np.all(a[0, col["top_zeros"]] == 0) and np.any(a[:, col["top_zeros"]] > 0) for a in (gas, ray))
        assert list(gas[:3, col["ties"], 0]) == [0.25, 0.25, 0.5][:nlayer]
        assert list(ray[:3, col["ties"], 0]) == [0.25, 0.5, 0.5][:nlayer]
        assert all(a[:, col["thin"]].sum(axis=0).max() < 0.5 for a in (gas, cld, ray))
        nan_cols = np.flatnonzero(np.isnan(gas).any(axis=(0, 2)))
        assert list(nan_cols) == [col["nan"]]                                  # exactly one column is excluded
        for at in fix["at_taus"]:
            for ig in range(ngauss):
                assert fix["%spa/%g/%d/pressure" % (t, at, ig)].shape == (3, 150)
                lv = fix["%spa/%g/%d/level" % (t, at, ig)]
                assert lv.shape == (3, 150) and lv.min() >= 0 and lv.max() <= nlayer
        for R in (0, 60):
            z = fix["%sheat/R%d/taugas" % (t, R)]
            assert z.shape == (nlayer, fix["%sheat/R%d/wavenumber" % (t, R)].size)
        assert np.isnan(fix[t + "heat/R60/tauray"]).all(axis=0).any()          # empty bins
    gas = fix["ck13/taugas"]
    assert not np.array_equal(gas[:, :, 0], gas[:, :, 2], equal_nan=True)      # differs per Gauss point
    assert fix["map/taugas"].shape == (4, 7, 3, 2, 2) and fix["map/cloud/w0"].shape == (4, 7, 3, 2)
    assert fix["map/level/pressure"].shape == (5, 3, 2)
    cum = np.cumsum(fix["map/taucld"][..., 0] * fix["map/cloud/w0"], axis=0)
    assert np.all(cum[0, :, 1, 0] > 0)                                         # the quirk facet: one zero, the top
    assert np.all(cum[-1, :, 2, 1] == 0) and np.all(cum[1, :, 0, 0] == 0)      # no cloud; a clear top
    for i, n in enumerate((None, 1, 0, 150)):
        count = int(fix["s13/optics/%d/count" % i])
        assert (count > 10) if n is None else (count == n)
        assert fix["s13/optics/%d/opd" % i].shape == (12,)


def test_the_walk_down_a_column_gives_the_reference_levels(fix):
    """The selection rule of csrc/attenuation.hip in numpy against the reference's np.unique / argmin indices."""
    nan_col = int(fix["cols"][list(fix["col_names"]).index("nan")])
    for name, (nlevel, ngauss) in SCENES.items():
        t = name + "/"
        for ig in range(ngauss):
            planes = (fix[t + "taugas"][:, :, ig], fix[t + "taucld"][:, :, ig] * fix[t + "cloud/w0"], fix[t + "tauray"][:, :, ig])
            for at in fix["at_taus"]:
                ref = fix["%spa/%g/%d/level" % (t, at, ig)]
                for k, d in enumerate(planes):
                    c = np.concatenate((np.zeros((1, 150)), np.cumsum(d, axis=0)))
                    best, gap, cb = np.zeros(150, dtype=int), np.abs(c[0] - at), c[0].copy()
                    for i in range(1, nlevel):
                        g = np.abs(c[i] - at)
                        take = (g < gap) | (c[i] == cb)
                        best, gap, cb = np.where(take, i, best), np.where(take, g, gap), np.where(take, c[i], cb)
                    ok = np.arange(150) != nan_col
                    assert np.array_equal(best[ok], ref[k, ok]), (name, ig, at, k)


def test_new_symbols_are_declared_and_exported():
    from picaso_amd import _lib
    from picaso_amd import build as b
    b.build(force=False)
    lib = _lib.load()
    names = _lib.declared_symbols()
    for n in NEW:
        assert n in names and hasattr(lib, n), n
    from picaso_amd import justdoit as jdi
    for n in ("photon_attenuation", "taumap", "heatmap_taus", "cloud_optics_1d"):
        assert callable(getattr(jdi, n))


def test_host_tables_agree_with_mean_regrid_and_the_reference(fix):
    from picaso_amd import justdoit as jdi
    from picaso_amd.attenuation import contiguous_window, nearest_wavelength, r_grid
    wno, R = fix["s13/wno"], int(fix["R"])
    wavenumber, plan = r_grid(wno, R)
    assert np.array_equal(wavenumber, jdi.mean_regrid(wno, wno, R=R)[0])
    assert np.array_equal(wavenumber, fix["s13/heat/R60/wavenumber"])
    idx = np.full(wno.size, -1)
    for j in range(plan.nbins):
        idx[plan.start[j]:plan.start[j + 1]] = j
    _, means = jdi.mean_regrid(wno, np.arange(wno.size, dtype=float), R=R)
    for j in range(plan.nbins):
        cols = np.flatnonzero(idx == j)
        assert (np.isnan(means[j]) and cols.size == 0) or means[j] == cols.mean(), j
    assert (plan.counts == 0).any()
    wave = 1e4 / wno
    for i, win in enumerate(fix["windows"]):
        lo, hi = contiguous_window(wno, win)
        assert hi - lo == int(fix["s13/optics/%d/count" % i])
        assert np.array_equal(np.arange(lo, hi), np.flatnonzero((wave > win[0]) & (wave < win[1])))
    with pytest.raises(Exception, match="not contiguous"):
        contiguous_window(np.array([2000.0, 5000.0, 2100.0]), (4.5, 5.5))
    for wl in fix["map/wavelengths"]:
        assert nearest_wavelength(fix["map/wno"], float(wl)) == int(fix["map/iw/%g" % wl])
    assert nearest_wavelength(np.array([8000.0, 10000.0, 40000.0 / 3.0]), 1.0) == 1
