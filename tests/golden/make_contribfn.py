"""Generate tests/golden/contribfn.npz by running the REFERENCE's own source (build container only):

    python tests/golden/make_contribfn.py

``justplotit.thermal_contribution`` (reference justplotit.py:1584-1643) and ``justplotit.transmission_contribution``
(:1697-1779) on synthetic ``full_output`` dictionaries: 150 wavenumbers (two full 64-lane tiles and a partial one) with a
gap and one isolated point, so that R = 60 leaves bins empty and one bin with a single column; 13, 3 and 2 levels (the
last two: fewer chords than waves, a single layer, an empty thermal result); a T(p) that is not isothermal, a cloud slab,
one opaque layer (dtau 1e4), one all-zero column and one column with a NaN in taugas.  The scenes and the numpy restatement
of get_transit_1d are tests/contribfn_cases.py's, which the tests share (they cannot import this file: it loads the reference).

Stored per scene ``s<nlevel>``: the inputs, the reference's thermal CF for tau_max 1 and 1e3 and its CF_bin (tau_max 1,
R = 60), the reference's transmission CF (its own arguments: layer pressure in bar, layer temperature, constants 1), and
the same transmission formula restated here in np.longdouble (``tr_cf_x80``) in the non-negative form of DESIGN.md.
Asserted: the float64 restatement of the transit depth equals the reference's get_transit_1d within nlevel 2^-52, no
column but the deliberate ones is NaN, and nothing lies in the denormal range where a comparison would be undefined."""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_shim  # noqa: E402
from contribfn_cases import COL_NAN, COL_OPAQUE, COL_ZERO, NWNO, scene, transit_terms  # noqa: E402

R_BIN = 60
TAU_MAXES = (1.0, 1e3)


def _justplotit():
    import matplotlib
    matplotlib.use("Agg")
    ref_shim.load("optics")                            # installs the shims and the `picaso` package stub
    for name in ("bokeh.layouts", "bokeh.models.annotations", "bokeh.transform", "scipy.stats.stats"):
        if name not in sys.modules:
            sys.modules[name] = ref_shim._Dummy(name)
    for name, mod in list(sys.modules.items()):       # `import a.b as c` reads the attribute b of a
        parent, _, child = name.rpartition(".")
        if parent and isinstance(sys.modules.get(parent), ref_shim._Dummy) and isinstance(mod, ref_shim._Dummy):
            setattr(sys.modules[parent], child, mod)
    return importlib.import_module("picaso.justplotit")


def main():
    jpi = _justplotit()
    fluxes = ref_shim.load("fluxes")
    import matplotlib.pyplot as plt
    store = {"nlevels": np.array([13, 3, 2]), "R": np.array(R_BIN), "tau_maxes": np.array(TAU_MAXES),
             "cols": np.array([COL_OPAQUE, COL_ZERO, COL_NAN])}
    worst = 0.0
    for nlevel in (13, 3, 2):
        full = scene(nlevel)
        nlayer, tag = nlevel - 1, "s%d/" % nlevel
        for k in ("taugas", "taucld", "tauray"):
            store[tag + k] = full[k][:, :, 0]
        store[tag + "wno"] = full["wavenumber"]
        for grp in ("layer", "level"):
            for k, v in full[grp].items():
                store["%s%s/%s" % (tag, grp, k)] = v
        # ---- thermal
        with np.errstate(all="ignore"):
            for tm in TAU_MAXES:
                if nlayer > 1:
                    cf = jpi.thermal_contribution(full, tau_max=tm, R=None)[2]
                else:
                    cf = np.zeros((0, NWNO))                  # the reference's figure cannot draw an empty plane
                plt.close("all")
                assert cf.shape == (nlayer - 1, NWNO)
                bad = np.isnan(cf).any(axis=0)
                assert not bad[np.arange(NWNO) != COL_NAN].any()
                assert not ((cf != 0) & (np.abs(cf) < 1e-290)).any()
                store["%sth_cf/%g" % (tag, tm)] = cf
            if nlayer > 1:
                cf_bin = jpi.thermal_contribution(full, tau_max=1.0, R=R_BIN)[2]
                plt.close("all")
                store[tag + "th_cf_bin"] = cf_bin
                centres = jpi.mean_regrid(full["wavenumber"], full["wavenumber"], R=R_BIN)[0]
                d = np.diff(centres)
                edges = np.concatenate(([centres[0] - d[0] / 2], centres[:-1] + d / 2.0, [centres[-1] + d[-1] / 2]))
                counts = np.histogram(full["wavenumber"], bins=edges)[0]
                assert (counts == 0).any() and (counts == 1).any(), counts
                nan_bin = np.searchsorted(edges, full["wavenumber"][COL_NAN], side="right") - 1
                want = (counts == 0) | ((np.arange(counts.size) == nan_bin) & np.isnan(cf[-1, COL_NAN]))
                assert np.array_equal(np.isnan(cf_bin[-1]), want)
                store[tag + "bin_counts"] = counts
                store[tag + "bin_wavenumber"] = centres
        # ---- transmission, the reference's arguments
        with np.errstate(all="ignore"):
            cf_ref = jpi.transmission_contribution(full, R=None)[3]
            plt.close("all")
            dtau = (full["taugas"][:, :, 0] + full["taucld"][:, :, 0]) + full["tauray"][:, :, 0]
            f_ref = fluxes.get_transit_1d(full["level"]["z"], full["level"]["dz"], nlevel, NWNO, 1, full["layer"]["mmw"], 1, 1,
                                          full["layer"]["pressure"], full["layer"]["temperature"],
                                          full["layer"]["column_density"], dtau)
            f64, _ = transit_terms(full, np.float64)
            _, d80 = transit_terms(full, np.longdouble)
            cf80 = d80 / d80.sum(axis=0)
        ok = np.arange(NWNO) != COL_NAN
        assert np.all(np.abs(f64[ok] - f_ref[ok]) <= nlevel * 2.0 ** -52 * np.abs(f_ref[ok]))
        assert np.isnan(f_ref[COL_NAN]) and np.isnan(cf80[:, COL_NAN]).all() and np.isnan(cf80[:, COL_ZERO]).all()
        ok[COL_ZERO] = False
        assert not np.isnan(cf80[:, ok]).any() and np.isfinite(cf80[:, COL_OPAQUE]).all()
        # a share the opaque layer hides is ~ exp(-5e3): 0 in float64, here and on the device; none may lie near the edge
        assert not ((cf80 > np.longdouble("1e-400")) & (cf80 < 1e-280)).any()
        cf80 = cf80.astype(np.float64)
        gap = np.nanmax(np.abs(cf_ref[:, ok] - cf80[:, ok]))
        worst = max(worst, gap)
        print("nlevel %d: max |ref - x80| = %.3e, smallest share %.3e, opaque column %s" % (
            nlevel, gap, cf80[:, ok][cf80[:, ok] > 0].min(), cf80[:, COL_OPAQUE]))
        store[tag + "tr_cf_ref"] = cf_ref
        store[tag + "tr_cf_x80"] = cf80
    path = os.path.join(HERE, "contribfn.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024), "largest |ref - x80| = %.3e" % worst)


if __name__ == "__main__":
    main()
