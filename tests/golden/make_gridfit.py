"""Generate tests/golden/gridfit.npz by running the REFERENCE's own grid fitter (build container only):

    python tests/golden/make_gridfit.py

The reference's ``analyze`` module does not import here (xarray, astropy, virga), so the definitions are taken from its
files with ``ast`` and compiled at generation time next to numpy, scipy and pandas; none of their text is stored.  From
``picaso/analyze.py`` the module functions ``custom_interp``, ``find_bounding_values``, ``get_last_dimension``,
``chi_squared`` and ``_finditem``, and the method bodies ``fit_grid``, ``get_chi_posteriors`` and ``transform_4_interp`` of
``GridFitter``, bound to a bare class; from ``picaso/justplotit.py`` ``mean_regrid``.

The inputs are tests/gridfit_cases.py's (rebuilt by the tests from integer arithmetic); the file holds arrays only:
  I<d>/probe        (40, ncol) every 17th column of custom_interp's result per goal, d = 1..5
  I<d>/digest       (40, 2) uint64: xor and wrapping sum of the bit patterns of ALL its columns (gridfit_cases.digest)
  I<d>/in_probe     a probe of the spectra and the goals
  I6/expected       (12, 257) custom_interp's results through its three-neighbour fallback
  F1/binned         (24, 60) mean_regrid of every model on the data set with empty bins
  F1b/binned        (24, 56) the same on the data set without them, and per (offset, dof) in o1/o0 x ndata/nparams:
  F1b/<o>_<dof>/chi2, shift, best, rank, post_<parameter> (fit_grid's chi_sqs, offsets, best_fits, rank, posteriors)
  F1b/shift_exact   (24) math.fsum(y - m) / ndata per model, next to curve_fit's shift
  F1b/shift_margin  (24) 2 |shift_ref - shift_exact|: the reference's own distance from exact arithmetic, doubled
  L1/binned, L1/logl  (200, 56), (200): custom_interp -> mean_regrid -> the likelihood expression of driver.py:326
"""
import ast
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gridfit_cases as gc          # noqa: E402

COMBOS = (("o1", True), ("o0", False)), ("ndata", "nparams")


def _reference():
    """The reference's functions and a bare fitter class carrying its three methods."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import itertools
    import pandas as pd
    import ref_shim
    import scipy as sp
    from scipy.interpolate import griddata
    from scipy.stats import binned_statistic
    ns = {"np": np, "pd": pd, "itertools": itertools, "cKDTree": sp.spatial.cKDTree, "optimize": sp.optimize,
          "griddata": griddata, "binned_statistic": binned_statistic}

    def take(fname, names, cls=None):
        path = os.path.join(ref_shim.REF_ROOT, "picaso", fname)
        with open(path) as fh:
            body = ast.parse(fh.read(), path).body
        if cls is not None:
            body = [n for n in body if isinstance(n, ast.ClassDef) and n.name == cls][0].body
        nodes = [n for n in body if isinstance(n, ast.FunctionDef) and n.name in names]
        assert sorted(n.name for n in nodes) == sorted(names), (fname, names)
        exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)

    take("justplotit.py", ["mean_regrid"])
    take("analyze.py", ["custom_interp", "find_bounding_values", "get_last_dimension", "chi_squared", "_finditem"])
    methods = ["fit_grid", "get_chi_posteriors", "transform_4_interp"]
    take("analyze.py", methods, cls="GridFitter")
    Bare = type("Bare", (), {m: ns[m] for m in methods})
    return ns, Bare


def _fitter(Bare, grid, wl, spectra, gp, nparams):
    f = Bare()
    f.list_of_files = {grid: list(range(spectra.shape[0]))}
    f.wavelength, f.spectra, f.grid_params = {grid: wl}, {grid: spectra}, {grid: gp}
    f.overview = {grid: {"num_params": nparams}}
    return f


def _prep(f, grid):
    sq, uniq, offset_pm, df = f.transform_4_interp(grid, add_ptchem=False)
    f.interp_params = {grid: {"offset_prior": offset_pm, "grid_parameters": df, "grid_parameters_unique": uniq,
                              "square_spectra_grid": sq}}


def main():
    ns, Bare = _reference()
    custom_interp, mean_regrid = ns["custom_interp"], ns["mean_regrid"]
    store = {}
    for d in range(1, 6):
        wl, spectra, gp, goals = gc.interp_case(d)
        f = _fitter(Bare, "g", wl, spectra, gp, d)
        _prep(f, "g")
        assert list(f.interp_params["g"]["grid_parameters_unique"]) == list(gc.NAMES[:d])
        out = np.stack([custom_interp(g, f, "g") for g in goals])
        assert out.shape == (gc.NGOALS_I, gc.NWAVE_I) and np.all(np.isfinite(out))
        store["I%d/probe" % d], store["I%d/digest" % d] = out[:, ::gc.PROBE], gc.digest(out)
        store["I%d/in_probe" % d] = np.concatenate([spectra[:, ::97].ravel(), goals.ravel()])
        print("I%d: %d models, |result| %.3g .. %.3g" % (d, spectra.shape[0], np.abs(out).min(), np.abs(out).max()))

    wl, spectra, gp, goals = gc.hole_case()
    f = _fitter(Bare, "g", wl, spectra, gp, 2)
    _prep(f, "g")
    assert np.isnan(f.interp_params["g"]["square_spectra_grid"][1, 1]).all()
    pts = np.stack([gp["planet_params"][n] for n in gc.NAMES[:2]], axis=1)
    with np.errstate(all="ignore"):
        out = np.stack([custom_interp(g, f, "g") for g in goals])
    for g in goals[:11]:                     # no ties among the neighbours: which three count does not hang on rounding
        dd = np.sort(np.sqrt(np.sum((pts - g) ** 2, axis=1)))
        assert np.all(np.diff(dd[:4]) > 1e-6 * dd[3]), dd
    assert np.all(np.isfinite(out[:11])) and np.all(np.isnan(out[11]))
    store["I6/expected"] = out
    store["I6/in_probe"] = np.concatenate([spectra[:, ::97].ravel(), goals.ravel()])

    wl, spectra, gp = gc.fit_case()
    names = list(gc.NAMES[:3])
    for data in ("F1", "F1b"):
        cen, wid, y, e = gc.fit_data(data)
        binned = np.stack([mean_regrid(wl, s, newx=cen)[1] for s in spectra])
        counts = np.histogram(wl, bins=np.concatenate(([cen[0] - (cen[1] - cen[0]) / 2], (cen[:-1] + cen[1:]) / 2,
                                                       [cen[-1] + (cen[-1] - cen[-2]) / 2])))[0]
        store[data + "/binned"], store[data + "/counts"] = binned, counts
        store[data + "/in_probe"] = np.concatenate([spectra[:, ::97].ravel(), cen, y, e])
        print(data, "bins of", sorted(set(counts.tolist())))
        if data == "F1":
            assert {0, 1, 63, 64, 65} <= set(counts.tolist()) and counts.max() > 1024 and cen.size == 60
            assert np.array_equal(np.isnan(binned), np.broadcast_to(counts == 0, binned.shape))
            continue
        assert counts.min() > 0
        store[data + "/shift_exact"] = np.array([math.fsum(y - m) / y.size for m in binned])
        for oname, offset in COMBOS[0]:
            for dof in COMBOS[1]:
                f = _fitter(Bare, "g", wl, spectra, gp, 3)
                f.data = {data: {"wlgrid_center": cen, "wlgrid_width": wid, "y_data": y, "e_data": e}}
                f.fit_grid("g", data, dof=dof, offset=offset)
                key = "%s/%s_%s/" % (data, oname, dof)
                chi2 = f.chi_sqs["g"][data]
                srt = np.sort(chi2)
                assert np.all(np.diff(srt) > 1e-6 * srt[1:]), "chi squares closer than 1e-6 relative"
                store[key + "chi2"], store[key + "best"] = chi2, f.best_fits["g"][data]
                store[key + "rank"] = f.rank["g"][data]
                store[key + "shift"] = f.offsets["g"][data] if offset else np.zeros(len(chi2))
                for n in names:
                    grid_vals, prob = f.posteriors["g"][data][n]
                    store[key + "post_" + n] = prob
                print(key, "chi2 %.4g .. %.4g" % (chi2.min(), chi2.max()))
        ref = store[data + "/o1_ndata/shift"]
        store[data + "/shift_margin"] = 2 * np.abs(ref - store[data + "/shift_exact"])
        print("curve_fit's shift vs exact: max rel %.2e" % np.max(np.abs(ref - store[data + "/shift_exact"]) / np.abs(ref)))

    goals, offset, scaling, err_inf = gc.loglike_case()
    cen, wid, y, e = gc.fit_data("F1b")
    f = _fitter(Bare, "g", wl, spectra, gp, 3)
    _prep(f, "g")
    binned = np.stack([mean_regrid(wl, custom_interp(g, f, "g"), newx=cen)[1] for g in goals])
    logl = np.empty(len(goals))
    for s in range(len(goals)):
        ydata_ = y + offset[s]
        ydata_ *= scaling[s]
        sigma = e ** 2 + err_inf[s]
        extra_term = np.log(2 * np.pi * sigma)
        logl[s] = -0.5 * np.sum((ydata_ - binned[s]) ** 2 / sigma + extra_term)
    store["L1/binned"], store["L1/logl"] = binned, logl
    store["L1/in_probe"] = np.concatenate([goals.ravel(), offset, scaling, err_inf])

    path = os.path.join(HERE, "gridfit.npz")
    np.savez_compressed(path, **store)
    size = os.path.getsize(path)
    print("wrote", path, "%.1f KB" % (size / 1024))
    assert size <= 1024 * 1024, "a committed file holds 1 MiB"


if __name__ == "__main__":
    main()
