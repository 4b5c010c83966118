"""What jdi.thermal_contribution / jdi.transmission_contribution need without a GPU: the fixture (tests/golden/contribfn.npz,
written by tests/golden/make_contribfn.py), the C entry points, and the bins of ``R``."""
import os

import numpy as np

from helpers import GOLDEN

NEW = ("picaso_thermal_cf_dev", "picaso_transit_cf_dev", "picaso_mean_regrid_plane_dev")


def test_fixture_loads_and_is_consistent():
    fix = np.load(os.path.join(GOLDEN, "contribfn.npz"))
    assert list(fix["nlevels"]) == [13, 3, 2] and len(set(int(c) // 64 for c in fix["cols"])) == 3
    for nlevel in fix["nlevels"]:
        t, nlayer = "s%d/" % nlevel, int(nlevel) - 1
        nwno = fix[t + "wno"].size
        assert nwno == 150 and np.all(np.diff(fix[t + "wno"]) > 0)
        for k in ("taugas", "taucld", "tauray", "tr_cf_ref", "tr_cf_x80"):
            assert fix[t + k].shape == (nlayer, nwno), k
        assert np.any(fix[t + "taucld"] > 0) and np.nanmax(fix[t + "taugas"]) == 1e4
        for k in ("pressure", "temperature", "column_density", "mmw"):
            assert fix["%slayer/%s" % (t, k)].shape == (nlayer,)
        for k in ("pressure", "temperature", "z", "dz"):
            assert fix["%slevel/%s" % (t, k)].shape == (nlevel,)
        assert np.ptp(fix[t + "level/temperature"]) > 100            # not isothermal
        for tm in fix["tau_maxes"]:
            assert fix["%sth_cf/%g" % (t, tm)].shape == (nlayer - 1, nwno)
        if nlayer > 1:
            counts = fix[t + "bin_counts"]
            assert fix[t + "th_cf_bin"].shape == (nlayer - 1, counts.size)
            assert (counts == 0).any() and (counts == 1).any()
        x80 = fix[t + "tr_cf_x80"]
        ok = ~np.isnan(x80[0])
        assert ok.sum() == nwno - 2 and np.allclose(x80[:, ok].sum(axis=0), 1.0, rtol=0, atol=1e-14)


def test_new_symbols_are_declared_and_exported():
    from picaso_amd import _lib
    from picaso_amd import build as b
    b.build(force=False)
    lib = _lib.load()
    names = _lib.declared_symbols()
    for n in NEW:
        assert n in names and hasattr(lib, n), n


def test_the_grid_of_R_is_mean_regrids():
    """``cf_grid``: the wavenumbers and the bin table of the reference's two mean_regrid calls (justplotit.py:1619-1625)."""
    from picaso_amd import justdoit as jdi
    from picaso_amd.contribution import cf_grid
    fix = np.load(os.path.join(GOLDEN, "contribfn.npz"))
    wno, R = fix["s13/wno"], int(fix["R"])
    wavenumber, plan = cf_grid(wno, R)
    assert np.array_equal(wavenumber, jdi.mean_regrid(wno, wno, R=R)[0])
    assert np.array_equal(wavenumber, fix["s13/bin_wavenumber"])
    assert np.array_equal(plan.counts, fix["s13/bin_counts"])
    # every column's bin by mean_regrid's own counting: bin j holds the columns [start[j], start[j + 1])
    idx = np.full(wno.size, -1)
    for j in range(plan.nbins):
        idx[plan.start[j]:plan.start[j + 1]] = j
    marks = np.arange(wno.size, dtype=float)
    _, means = jdi.mean_regrid(wno, marks, newx=wavenumber)
    for j in range(plan.nbins):
        cols = np.flatnonzero(idx == j)
        assert (np.isnan(means[j]) and cols.size == 0) or means[j] == cols.mean(), j
    assert np.array_equal(np.diff(plan.start), plan.counts)
