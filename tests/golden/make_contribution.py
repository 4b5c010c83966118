"""Generate tests/golden/contribution.npz by running the REFERENCE's own source (build container only):

    python tests/golden/make_contribution.py

``optics.compute_opacity(..., return_mode=True)`` (reference optics.py:123-319) on the committed synthetic_opacities.db
with the duck-typed atmosphere of make_golden.make_optics (both query methods, raman=2), and on the bare premixed
``RetrieveCKs`` of make_golden.make_ck (continuum, rayleigh and cloud keys only); then get_contribution's column pass
(justdoit.py:1272-1286) restated: a zero row on top of the cumulative sum, ``np.interp`` per column for several at_tau.
Stored per case: the species keys in order, the planes, the cumulative sums and the pressures."""
import os
import sqlite3
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ref_shim  # noqa: E402
from make_golden import _ref_colden, _ref_weights  # noqa: E402

AT_TAUS = (1.0, 0.1, 0.0, 30.0)


def _atm(og, nlayer, nlevel):
    import pandas as pd
    plevel_bar, tlevel, gravity = og["in/plevel_bar"], og["in/tlevel"], float(og["in/gravity"])
    mix = {k: og["in/mix/" + k] for k in ("H2", "He", "H2O", "CH4")}
    weights = _ref_weights(tuple(mix))
    atm = types.SimpleNamespace()
    atm.c = types.SimpleNamespace(nlayer=nlayer, nlevel=nlevel, pconv=1e6, k_b=1.380649e-16,
                                  amu=1.66053906660e-24, rgas=8.31446261815324)
    atm.planet = types.SimpleNamespace(gravity=gravity)
    p = plevel_bar * 1e6
    atm.level = {"pressure": p, "temperature": tlevel}
    mmw_lvl = sum(mix[k] * weights[k] for k in mix)
    opd = og["in/cld_opd"].copy()
    atm.layer = {"pressure": np.sqrt(p[1:] * p[:-1]), "temperature": 0.5 * (tlevel[1:] + tlevel[:-1]),
                 "mmw": 0.5 * (mmw_lvl[1:] + mmw_lvl[:-1]), "colden": _ref_colden(p, tlevel, mmw_lvl, gravity),
                 "electrons": np.zeros(nlayer),
                 "mixingratios": pd.DataFrame({k: 0.5 * (v[1:] + v[:-1]) for k, v in mix.items()}),
                 "cloud": {"opd": opd, "w0": og["in/cld_w0"].copy(), "g0": og["in/cld_g0"].copy()}}
    # the orders ATMSETUP gives a profile with the columns H2, He, H2O, CH4 (the tests' bundle): the keys' order
    atm.molecules = np.array(["H2", "H2O", "CH4"])
    atm.continuum_molecules = [["H2", "H2"], ["H2", "He"], ["H2", "CH4"]]
    atm.rayleigh_molecules = ["H2", "He", "H2O", "CH4"]
    return atm


def _store_case(store, tag, taus, plevel_bar):
    """get_contribution's column pass as the reference writes it (justdoit.py:1272-1286, find_press :1289-1294)."""
    store[tag + "/keys"] = np.array(list(taus.keys()))
    for k, t in taus.items():
        t = np.asarray(t)
        cum = np.zeros((t.shape[0] + 1, t.shape[1]))
        cum[1:, :] = np.cumsum(t, axis=0)
        store["%s/taus/%s" % (tag, k)] = t
        store["%s/cum/%s" % (tag, k)] = cum
        for a in AT_TAUS:
            store["%s/p_at/%g/%s" % (tag, a, k)] = np.array(
                [np.interp([a], cum[:, iw], plevel_bar)[0] for iw in range(t.shape[1])])


def main():
    sqlite3.register_adapter(np.int64, int)
    optics = ref_shim.load("optics")
    og = np.load(os.path.join(HERE, "optics.npz"))
    ck = np.load(os.path.join(HERE, "ck.npz"))
    db = os.path.join(HERE, "synthetic_opacities.db")
    plevel_bar = og["in/plevel_bar"]
    nlevel = plevel_bar.size
    nlayer = nlevel - 1
    store = {"at_taus": np.array(AT_TAUS)}
    raman_file = os.path.join(ref_shim.REF_ROOT, "reference", "opacities", "raman.txt")
    for qm in ("nearest", "linear"):
        opa = optics.RetrieveOpacities(db, raman_file, query_method=qm)
        atm = _atm(og, nlayer, nlevel)
        opa.get_opacities(atm)
        taus = optics.compute_opacity(atm, opa, ngauss=1, stream=2, delta_eddington=True, test_mode=None, raman=2,
                                      return_mode=True)
        _store_case(store, qm, taus, plevel_bar)
    # premixed correlated-k (make_golden.make_ck's bare RetrieveCKs): continuum, rayleigh and cloud keys only
    opa = object.__new__(optics.RetrieveCKs)
    press, temps, nc_p = ck["in/press"], ck["in/temps"], ck["in/nc_p"]
    opa.pressures = np.concatenate([press[:n] for n in nc_p])
    opa.temps = np.concatenate([[t] * n for t, n in zip(temps, nc_p)])
    opa.nc_p, opa.kappa = nc_p, ck["in/kappa"]
    opa.continuum_db, opa.cia_temps = db, ck["in/cia_temps"]
    opa.wno = og["in/wno"]
    opa.nwno, opa.ngauss, opa.gauss_wts = opa.wno.size, ck["in/gauss_wts"].size, ck["in/gauss_wts"]
    rayleigh = ref_shim.load("rayleigh")
    ray = rayleigh.Rayleigh(opa.wno)
    opa.rayleigh_opa = {m: ray.compute_sigma(m) for m in ("H2", "He", "CH4", "H2O")}
    atm = _atm(og, nlayer, nlevel)
    opa.get_pre_mix_ck(atm)
    opa.get_continuum(atm)
    taus = optics.compute_opacity(atm, opa, ngauss=opa.ngauss, stream=2, delta_eddington=True, test_mode=None,
                                  raman=2, return_mode=True)
    _store_case(store, "ck", taus, plevel_bar)
    path = os.path.join(HERE, "contribution.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024),
          {qm: list(store[qm + "/keys"]) for qm in ("nearest", "linear", "ck")})


if __name__ == "__main__":
    main()
