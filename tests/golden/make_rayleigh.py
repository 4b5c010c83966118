"""Generate tests/golden/rayleigh.npz and rayleigh_fine.npz by running the REFERENCE's own source (build container only):

    python tests/golden/make_rayleigh.py

Arrays only.  Per wavenumber grid: ``<grid>/wno`` (the stored columns), ``<grid>/index`` (their positions in the full grid),
and for every name of ``names`` the reference's ``Rayleigh(wno).compute_sigma(name)`` as ``<grid>/sigma/<name>`` and the
refractive index its species method (or ``generic``) returns as ``<grid>/eta/<name>``.  ``names``: the 39 of
``rayleigh_molecules`` (stored as ``molecules``), N2O (a fit of its own, not in the list), C2H6 (a King factor, no
polarisability) and Ar (in neither table).

Grids:
  db    the wavenumber grid of synthetic_opacities.db, every column
  fine  linspace(2000, 33333, 100000): the first and last 50 columns and a seeded sample of 2 000 (rayleigh_fine.npz)
  wide  linspace(50, 60000, 20001), which crosses every piecewise limit of the fits (H2O above 17.6 micron is exactly
        zero): the first and last 50 columns, the 20 columns on either side of each of the ten limits, and a seeded sample
        of 600.  All 20 001 columns of 42 names would be 13 MB; a committed file holds 1 MiB.

``planes/...``: the reference's ``RetrieveOpacities(synthetic_opacities.db, raman.txt, query_method=...)`` -- which computes
all 39 species itself and never reads the database's ``rayleigh`` table -- driven with the duck-typed atmosphere of
make_contribution._atm plus the mixing-ratio columns CO2, N2, NH3, CO, Na and K.  The database has no molecular rows for
these: they enter through ``rayleigh_molecules`` (ATMSETUP.get_needed_continuum's own answer, stored) and the mean
molecular weight.  Stored: the inputs (``planes/in/...``), the 13 ``compute_opacity`` planes and TAURAY (the 'rayleigh'
entry of ``return_mode=True``) per query method."""
import os
import sqlite3
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ref_shim  # noqa: E402
from make_contribution import _atm  # noqa: E402
from make_golden import _ref_colden, _ref_weights  # noqa: E402

EXTRA_NAMES = ("N2O", "C2H6", "Ar")
LIMITS_UM = (0.2540, 0.2753, 0.325, 0.360, 0.46816, 0.4801, 0.633, 2.0576, 2.0586, 17.60)
PLANES = ("dtau", "tau", "w0", "cosb", "ftau_cld", "ftau_ray", "gcos2", "dtau_og", "tau_og", "w0_og", "cosb_og",
          "w0_no_raman", "f_deltaM")
EXTRA_MIX = {"CO2": (2e-4, 6e-4), "N2": (1e-3, 4e-3), "NH3": (5e-5, 2e-4), "CO": (3e-4, 1e-4), "Na": (2e-6, 1e-6),
             "K": (1e-7, 3e-7)}          # (top, bottom) mixing ratio, linear in level index


def _store_grid(store, rayleigh, tag, wno, index, names):
    ray = rayleigh.Rayleigh(wno)
    store[tag + "/wno"], store[tag + "/index"] = wno[index], index
    for name in names:
        method = getattr(ray, name, None)
        with np.errstate(all="ignore"):
            eta = (method() if method is not None else ray.generic(name))[0]
            store["%s/sigma/%s" % (tag, name)] = np.asarray(ray.compute_sigma(name))[index]
        store["%s/eta/%s" % (tag, name)] = np.asarray(eta)[index]


def _sample(rng, n, count, ends=50, around=()):
    keep = set(range(ends)) | set(range(n - ends, n)) | set(rng.choice(n, size=count, replace=False).tolist())
    for lo, hi in around:
        keep |= set(range(max(lo, 0), min(hi, n)))
    return np.array(sorted(keep))


def _many_species_atm(og, nlayer, nlevel, atmsetup, available_ray):
    """make_contribution._atm with the extra columns: mixing ratios, mean molecular weight, column density and the
    Rayleigh list redone for the ten species."""
    import pandas as pd
    atm = _atm(og, nlayer, nlevel)
    mix = {k: og["in/mix/" + k] for k in ("H2", "He", "H2O", "CH4")}
    for k, (top, bottom) in EXTRA_MIX.items():
        mix[k] = np.linspace(top, bottom, nlevel)
    weights = _ref_weights(tuple(mix))
    mmw_lvl = sum(mix[k] * weights[k] for k in mix)
    atm.layer["mmw"] = 0.5 * (mmw_lvl[1:] + mmw_lvl[:-1])
    atm.layer["colden"] = _ref_colden(atm.level["pressure"], og["in/tlevel"], mmw_lvl, float(og["in/gravity"]))
    atm.layer["mixingratios"] = pd.DataFrame({k: 0.5 * (v[1:] + v[:-1]) for k, v in mix.items()})
    with_opacity = atm.molecules
    atm.molecules = np.array(list(mix))                 # the profile's columns, as ATMSETUP.get_profile leaves them
    atmsetup.ATMSETUP.get_needed_continuum(atm, available_ray, ["H2H2", "H2He", "H2CH4"])
    assert atm.continuum_molecules == [["H2", "H2"], ["H2", "He"], ["H2", "CH4"]]
    atm.molecules = with_opacity
    return atm, mix, weights


def main():
    sqlite3.register_adapter(np.int64, int)
    optics, rayleigh, atmsetup = ref_shim.load("optics"), ref_shim.load("rayleigh"), ref_shim.load("atmsetup")
    og = np.load(os.path.join(HERE, "optics.npz"))
    db = os.path.join(HERE, "synthetic_opacities.db")
    molecules = rayleigh.Rayleigh(np.ones(1)).rayleigh_molecules
    names = list(molecules) + list(EXTRA_NAMES)
    rng = np.random.default_rng(20261)
    store = {"molecules": np.array(molecules), "names": np.array(names)}
    _store_grid(store, rayleigh, "db", og["in/wno"], np.arange(og["in/wno"].size), names)
    wide = np.linspace(50.0, 60000.0, 20001)
    edge = [int(np.searchsorted(wide, 1e4 / lim)) for lim in LIMITS_UM]
    _store_grid(store, rayleigh, "wide", wide, _sample(rng, wide.size, 600, around=[(e - 20, e + 20) for e in edge]), names)
    fine_store = {"names": np.array(names)}
    fine = np.linspace(2000.0, 33333.0, 100000)
    _store_grid(fine_store, rayleigh, "fine", fine, _sample(rng, fine.size, 2000), names)

    plevel_bar = og["in/plevel_bar"]
    nlevel = plevel_bar.size
    nlayer = nlevel - 1
    raman_file = os.path.join(ref_shim.REF_ROOT, "reference", "opacities", "raman.txt")
    for qm in ("nearest", "linear"):
        opa = optics.RetrieveOpacities(db, raman_file, query_method=qm)
        assert list(opa.rayleigh_molecules) == molecules
        atm, mix, weights = _many_species_atm(og, nlayer, nlevel, atmsetup, opa.rayleigh_molecules)
        opa.get_opacities(atm)
        out = optics.compute_opacity(atm, opa, ngauss=1, stream=2, delta_eddington=True, test_mode=None, raman=2)
        for nm, arr in zip(PLANES, out):
            store["planes/%s/%s" % (qm, nm)] = np.asarray(arr)[:, :, 0]
        atm, _, _ = _many_species_atm(og, nlayer, nlevel, atmsetup, opa.rayleigh_molecules)
        opa.get_opacities(atm)
        taus = optics.compute_opacity(atm, opa, ngauss=1, stream=2, delta_eddington=True, test_mode=None, raman=2,
                                      return_mode=True)
        store["planes/%s/tauray" % qm] = np.asarray(taus["rayleigh"])
    store["planes/rayleigh_molecules"] = np.array(atm.rayleigh_molecules)
    store["planes/in/columns"] = np.array(list(mix))
    for k, v in mix.items():
        store["planes/in/mix/" + k] = v
        store["planes/in/weight/" + k] = np.array(weights[k])
    for k in ("plevel_bar", "tlevel", "gravity", "cld_opd", "cld_w0", "cld_g0"):
        store["planes/in/" + k] = og["in/" + k]
    store["planes/in/colden"] = atm.layer["colden"]
    for fname, st in (("rayleigh.npz", store), ("rayleigh_fine.npz", fine_store)):
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **st)
        size = os.path.getsize(path)
        print("wrote", path, "%.1f KB" % (size / 1024))
        assert size <= 1024 * 1024, "a committed file holds 1 MiB"
    print("rayleigh_molecules of the many-species atmosphere:", list(atm.rayleigh_molecules))


if __name__ == "__main__":
    main()
