"""Opacity objects compute their own Rayleigh cross sections (picaso_amd/rayleigh.py) when neither the caller nor the
database supplies them -- through the device path: TAURAY and the 13 ``compute_opacity`` planes, ``spectrum`` /
``spectrum_batch`` / sharded spectra, correlated-k tables read from files, ``get_contribution``.

The database is tests/golden/synthetic_opacities.db with its ``rayleigh`` table dropped: what the reference's
databases look like (``header``, ``molecular``, ``continuum`` only).  Before picaso_amd/rayleigh.py such a database gave
``rayleigh_molecules == []``, TAURAY = 0, ftau_ray = 0/0 in every cloud-free layer and no lean cloud-free path
(test_database_without_rayleigh_table failed with "TAURAY must be > 0 everywhere").

Tolerances: planes against planes 1e-10 elementwise with the NaN pattern exact -- what tests/test_optics.py holds against
the reference's planes (the cross sections themselves differ by at most the bound of tests/test_rayleigh_host.py, and
more Rayleigh species only add terms of the same sum); the 'rayleigh' species plane against TAURAY 1e-13
(tests/test_contribution_gpu.py's bound between the species planes and the sums)."""
import os
import shutil
import sqlite3

import numpy as np
import pytest

import test_ck_readers as tck
import test_optics as topt
from helpers import GOLDEN
from test_rayleigh_host import _bound

pytestmark = pytest.mark.gpu
DB = topt.DB
NAMES = topt.NAMES


@pytest.fixture(scope="module")
def og():
    return np.load(os.path.join(GOLDEN, "optics.npz"))


@pytest.fixture(scope="module")
def ray_gold():
    return np.load(os.path.join(GOLDEN, "rayleigh.npz"))


@pytest.fixture(scope="module")
def bare_db(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("db") / "no_rayleigh.db")
    shutil.copy(DB, path)
    conn = sqlite3.connect(path)
    conn.execute("DROP TABLE rayleigh")
    conn.commit()
    conn.close()
    return path


def _planes(case, opa, raman=2):
    """(the 13 planes, TAURAY, atm) of ``case`` with the ATMSETUP sequence of tests/test_optics.py"""
    from picaso_amd import optics as px
    from picaso_amd.atmsetup import ATMSETUP
    atm = ATMSETUP(case.inputs)
    atm.planet.gravity = case.inputs["planet"]["gravity"]
    atm.get_profile(); atm.get_mmw(); atm.get_altitude(); atm.get_column_density()
    atm.get_needed_continuum(opa.rayleigh_molecules, opa.avail_continuum)
    atm.get_clouds(opa.wno)
    atm.molecules = np.array([m for m in atm.molecules if m in opa.molecules])
    opa.get_opacities(atm)
    out = px.compute_opacity(atm, opa, ngauss=1, stream=2, delta_eddington=True, test_mode=None, raman=raman,
                             full_output=True)
    return {nm: arr[:, :, 0] for nm, arr in zip(NAMES, out)}, atm.tauray[:, :, 0], atm


def _max_rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b) / np.where(np.abs(b) > 0, np.abs(b), 1.0)))


def test_database_without_rayleigh_table(og, bare_db):
    """THE test that fails without picaso_amd/rayleigh.py: opannection on a database without a ``rayleigh`` table."""
    from picaso_amd import justdoit as jdi
    bare = jdi.opannection(filename_db=bare_db, query_method="linear")
    tab = jdi.opannection(filename_db=DB, query_method="linear")
    case = topt._bundle(og, jdi, None, True, 2, 2)
    got, tauray, atm = _planes(case, bare)
    print("rayleigh_molecules of the opacity object: %d, of the atmosphere: %s; TAURAY min %.3g max %.3g"
          % (len(bare.rayleigh_molecules), atm.rayleigh_molecules, tauray.min(), tauray.max()))
    assert np.all(tauray > 0), "TAURAY must be > 0 everywhere: min %g, rayleigh_molecules %s" % (
        tauray.min(), atm.rayleigh_molecules)
    assert not np.isnan(got["ftau_ray"]).any(), "ftau_ray has %d NaN" % int(np.isnan(got["ftau_ray"]).sum())
    assert len(bare.rayleigh_molecules) == 39 and atm.rayleigh_molecules == ["H2", "He", "H2O", "CH4"]
    want, tauray_tab, _ = _planes(topt._bundle(og, jdi, None, True, 2, 2), tab)
    print("TAURAY computed against the table's: max rel err %.3g" % _max_rel(tauray, tauray_tab))
    assert topt._close(tauray, tauray_tab, 1e-10)
    for nm in NAMES:
        print("%-12s max rel err %.3g" % (nm, _max_rel(np.nan_to_num(got[nm]), np.nan_to_num(want[nm]))))
        assert topt._close(got[nm], want[nm], 1e-10), nm


def _many_case(jdi, g):
    case = jdi.inputs()
    case.phase_angle(0)
    case.gravity(gravity=float(g["planes/in/gravity"]))
    prof = {"pressure": g["planes/in/plevel_bar"], "temperature": g["planes/in/tlevel"]}
    for k in g["planes/in/columns"]:
        prof[str(k)] = g["planes/in/mix/" + str(k)]
    case.atmosphere(df=prof)
    case.clouds(df={"opd": g["planes/in/cld_opd"], "w0": g["planes/in/cld_w0"], "g0": g["planes/in/cld_g0"]})
    case.approx(raman="none", delta_eddington=True)
    return case


@pytest.mark.parametrize("qm", ["nearest", "linear"])
def test_many_species_against_the_reference(ray_gold, bare_db, qm):
    """Ten Rayleigh species (H2, He, H2O, CH4, CO2, N2, NH3, CO, Na, K) against the reference's own planes."""
    from picaso_amd import justdoit as jdi
    opa = jdi.opannection(filename_db=bare_db, query_method=qm)
    got, tauray, atm = _planes(_many_case(jdi, ray_gold), opa)
    assert atm.rayleigh_molecules == [str(m) for m in ray_gold["planes/rayleigh_molecules"]]
    assert len(atm.rayleigh_molecules) == 10
    assert np.allclose(atm.layer["colden"], ray_gold["planes/in/colden"], rtol=1e-12)
    print("%s tauray max rel err %.3g" % (qm, _max_rel(tauray, ray_gold["planes/%s/tauray" % qm])))
    assert topt._close(tauray, ray_gold["planes/%s/tauray" % qm], 1e-10)
    for nm in NAMES:
        ref = ray_gold["planes/%s/%s" % (qm, nm)]
        print("%s %-12s max rel err %.3g" % (qm, nm, _max_rel(np.nan_to_num(got[nm]), np.nan_to_num(ref))))
        assert topt._close(got[nm], ref, 1e-10), (qm, nm)


def _clear_case(jdi, og, dt=0.0):
    case = jdi.inputs()
    case.phase_angle(0)
    case.gravity(gravity=float(og["in/gravity"]), radius=7.1e9, mass=1.9e30)
    prof = {"pressure": og["in/plevel_bar"], "temperature": og["in/tlevel"] + dt}
    for k in ("H2", "He", "H2O", "CH4"):
        prof[k] = og["in/mix/" + k]
    case.atmosphere(df=prof)
    case.star(relative_flux=1.0 + 0.3 * np.sin(np.arange(len(og["in/wno"])) / 7.0), radius=6.9e10, semi_major=7.5e12)
    case.approx(raman="none", delta_eddington=True)
    return case


def _same_result(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_spectrum_end_to_end(og, bare_db):
    from picaso_amd import planes
    from picaso_amd import justdoit as jdi
    from picaso_amd.rayleigh import Rayleigh
    from picaso_amd.spectrum import _setup_atmosphere
    calc = "reflected+thermal"
    opa = jdi.opannection(filename_db=bare_db, query_method="linear")
    r = Rayleigh(opa.wno)
    given = jdi.opannection(filename_db=bare_db, query_method="linear",
                            rayleigh_opa={m: r.compute_sigma(m) for m in r.rayleigh_molecules})
    out = _clear_case(jdi, og).spectrum(opa, calculation=calc, devices=1)
    assert np.isfinite(out["albedo"]).all() and (out["albedo"] > 0).all() and np.isfinite(out["thermal"]).all()
    # the computed and the supplied path meet in the same device tables
    _same_result(out, _clear_case(jdi, og).spectrum(given, calculation=calc, devices=1))
    # spectrum_batch of two such cases equals the single calls
    cases = [_clear_case(jdi, og), _clear_case(jdi, og, dt=25.0)]
    batch = jdi.spectrum_batch(cases, opa, calculation=calc)
    for c, b in zip(cases, batch):
        _same_result(c.spectrum(opa, calculation=calc), b)
    assert not np.array_equal(batch[0]["thermal"], batch[1]["thermal"])
    # wavelength blocks on contexts of their own (device 0 three times: every box), every species' row sliced
    _same_result(out, _clear_case(jdi, og).spectrum(opa, calculation=calc, devices=[0, 0, 0]))
    assert all(len(s._ray) == 39 for _, _, s in opa._shards[(0, 0, 0)])
    # a cloud-free case takes the lean plane set
    case = _clear_case(jdi, og)
    atm = _setup_atmosphere(case.inputs, opa, opa.wno)
    assert atm.rayleigh_molecules == ["H2", "He", "H2O", "CH4"]
    assert planes.choose_1d(case.inputs, atm, opa.nwno, 1, calc).lean


def test_spectrum_sharded_over_the_visible_gpus(og, bare_db):
    from picaso_amd import _lib
    from picaso_amd import justdoit as jdi
    n = _lib.device_count()
    if n < 2:
        pytest.skip("one GPU visible (the sharded path on one device: test_spectrum_end_to_end)")
    opa = jdi.opannection(filename_db=bare_db, query_method="linear")
    want = _clear_case(jdi, og).spectrum(opa, calculation="reflected+thermal")
    _same_result(want, _clear_case(jdi, og).spectrum(opa, calculation="reflected+thermal", devices=n))


def test_correlated_k_from_files(og, ray_gold, tmp_path, monkeypatch):
    """opannection(method='resortrebin') without rayleigh_opa=: TAURAY as with the fixture's cross sections supplied."""
    from picaso_amd import justdoit as jdi
    wno = np.sort(og["in/wno"])
    assert np.array_equal(wno, ray_gold["db/wno"])
    ref, _ = tck._refdata(tmp_path, wno)
    cdb = str(tmp_path / "cont.db")
    tck._cont_db_on(cdb, wno)
    d = tmp_path / "resortrebin"
    d.mkdir()
    for m, a in tck._tables(wno.size, 8, seed=11).items():
        np.save(d / ("%s_1460.npy" % m), a)
    monkeypatch.setenv("picaso_refdata", ref)
    molecules = [str(m) for m in ray_gold["molecules"]]
    computed = jdi.opannection(method="resortrebin", ck_db=str(d), filename_db=cdb)
    given = jdi.opannection(method="resortrebin", ck_db=str(d), filename_db=cdb,
                            rayleigh_opa={m: ray_gold["db/sigma/" + m] for m in molecules})
    assert computed.rayleigh_molecules == molecules == given.rayleigh_molecules and computed.on_fly

    def tauray(o):
        case = _clear_case(jdi, og)
        fo = case.spectrum(o, calculation="reflected+thermal", full_output=True)["full_output"]
        return np.asarray(fo["tauray"]).reshape(len(og["in/tlevel"]) - 1, wno.size, -1)[:, :, 0]
    a, b = tauray(computed), tauray(given)
    bound = max(_bound(ray_gold["db/eta/" + m]) for m in ("H2", "He", "H2O", "CH4"))
    print("correlated-k TAURAY: max rel err %.3g (bound %.3g)" % (_max_rel(a, b), bound))
    assert np.all(b > 0) and _max_rel(a, b) <= bound


def test_contribution_rayleigh_plane(og, bare_db):
    from picaso_amd import justdoit as jdi
    opa = jdi.opannection(filename_db=bare_db, query_method="linear")
    case = topt._bundle(og, jdi, None, True, 2, 2)
    ray = jdi.get_contribution(case, opa)["taus_per_layer"]["rayleigh"]
    _, tauray, _ = _planes(topt._bundle(og, jdi, None, True, 2, 2), opa)
    assert ray.shape == tauray.shape and np.all(ray > 0)
    print("'rayleigh' species plane against TAURAY: max rel err %.3g" % _max_rel(ray, tauray))
    assert topt._close(ray, tauray, 1e-13)
