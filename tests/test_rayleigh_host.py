"""picaso_amd.rayleigh (host-side numpy) against the reference's own cross sections (tests/golden/rayleigh.npz and
rayleigh_fine.npz, written by tests/golden/make_rayleigh.py), and the rule of the opacity readers: cross sections the
caller supplies win, then a ``rayleigh`` table of the database, else they are computed.

The bound per species is ``max(1e-14, 8 eps / min|eta - 1|)`` (eps = 2.2e-16; the minimum over the stored grid points
of that species with eta != 1): the cross section goes as (eta^2 - 1)^2 with eta - 1 between 3.5e-5 (He) and 1e-3, so ONE
rounding of eta moves it by about 4 eps / (eta - 1).  Where the reference is exactly zero (H2O above 17.6 micron) the
result is exactly zero.  Largest relative error found, all names: 0 on each of the three grids (the stored values are
reproduced bit for bit), and 0 against the four rows of the ``rayleigh`` table of synthetic_opacities.db."""
import os
import shutil
import sqlite3

import numpy as np
import pytest

import test_ck_readers as tck
from helpers import GOLDEN

DB = os.path.join(GOLDEN, "synthetic_opacities.db")
EPS = 2.2e-16
GRIDS = {"db": None, "fine": np.linspace(2000.0, 33333.0, 100000), "wide": np.linspace(50.0, 60000.0, 20001)}


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(GOLDEN, "rayleigh.npz")))
    g.update(np.load(os.path.join(GOLDEN, "rayleigh_fine.npz")))
    return g


def _bound(eta):
    d = np.abs(eta[eta != 1] - 1)
    return max(1e-14, 8 * EPS / d.min()) if d.size else 1e-14


def _check(sigma, ref, eta, what):
    """(largest relative error) of ``sigma`` against the reference's ``ref``; asserts zeros, finiteness and the bound"""
    zero = ref == 0
    assert np.all(np.isfinite(sigma)), what
    assert np.all(sigma[zero] == 0), what
    err = float(np.max(np.abs(sigma[~zero] - ref[~zero]) / np.abs(ref[~zero]))) if (~zero).any() else 0.0
    print("%-12s max rel err %.3g (bound %.3g)" % (what, err, _bound(eta)))
    assert err <= _bound(eta), (what, err, _bound(eta))
    return err


def test_surface_and_species_list(gold):
    from picaso_amd.rayleigh import Rayleigh
    wno = gold["db/wno"]
    r = Rayleigh(wno)
    assert r.rayleigh_molecules == list(gold["molecules"]) and len(r.rayleigh_molecules) == 39
    assert r.rayleigh_molecules == list(r.polarisabilities.keys())
    assert r.wno is wno and np.array_equal(r.wavelength, 1e4 / wno)
    assert r.n_ref == (101325.0 / (1.380649e-23 * 273.15)) * 1.0e-6
    assert set(r.king_correction_no_wave) == {"O3", "CO", "C2H2", "C2H6", "OCS", "CH3Cl", "H2S", "SO2"}
    assert "N2O" not in r.rayleigh_molecules and "Ar" not in r.polarisabilities


@pytest.mark.parametrize("grid", ["db", "fine", "wide"])
def test_compute_sigma_against_the_reference(gold, grid):
    from picaso_amd.rayleigh import Rayleigh
    index = gold[grid + "/index"]
    full = gold["db/wno"] if GRIDS[grid] is None else GRIDS[grid]
    assert np.array_equal(full[index], gold[grid + "/wno"])
    r = Rayleigh(full)
    names = list(gold["names"])
    assert names[:39] == r.rayleigh_molecules and {"N2O", "Ar"} <= set(names[39:])
    worst = 0.0
    for name in names:
        sigma = r.compute_sigma(name)
        assert sigma.shape == full.shape and np.all(np.isfinite(sigma)), name
        eta = r.refractive_index(name)[0]
        assert np.array_equal(eta[index] == 1, gold["%s/eta/%s" % (grid, name)] == 1), name
        worst = max(worst, _check(sigma[index], gold["%s/sigma/%s" % (grid, name)], gold["%s/eta/%s" % (grid, name)],
                                  grid + "/" + name))
    print("grid %s: largest relative error %.3g" % (grid, worst))
    if grid == "wide":      # every piecewise limit is crossed, and water above 17.6 micron scatters nothing
        wl = 1e4 / gold["wide/wno"]
        for lim in (0.2540, 0.2753, 0.325, 0.360, 0.46816, 0.4801, 0.633, 2.0576, 2.0586, 17.60):
            assert (wl < lim).sum() >= 20 and (wl > lim).sum() >= 20
        assert np.all(gold["wide/sigma/H2O"][wl > 17.60] == 0) and np.all(gold["wide/sigma/H2O"][wl <= 17.60] > 0)


def _db_rayleigh():
    from picaso_amd import optics as px
    conn = sqlite3.connect(DB)
    rows = {m: px._convert_array(b) for m, b in conn.execute("SELECT molecule, opacity FROM rayleigh")}
    conn.close()
    return rows


def test_the_rayleigh_table_of_the_synthetic_database(gold):
    from picaso_amd.rayleigh import Rayleigh
    rows = _db_rayleigh()
    assert list(rows) == ["H2", "He", "CH4", "H2O"]
    r = Rayleigh(gold["db/wno"])
    for m, ref in rows.items():
        _check(r.compute_sigma(m), ref, gold["db/eta/" + m], "table/" + m)


# ---- the readers' rule, without a GPU ---------------------------------------------------------------------------------
class _FakeDev:
    """Stand-in for DeviceArray (as tests/test_inputs_host.py): keeps what was uploaded."""

    def __init__(self, arr):
        self.host = np.array(arr)
        self.shape = self.host.shape

    @classmethod
    def from_host(cls, arr, ctx=None):
        return cls(arr)

    def to_host(self):
        return self.host


@pytest.fixture
def px(monkeypatch):
    from picaso_amd import optics
    monkeypatch.setattr(optics, "DeviceArray", _FakeDev)
    return optics


@pytest.fixture
def bare_db(tmp_path):
    """synthetic_opacities.db as the reference's databases are: no ``rayleigh`` table"""
    path = str(tmp_path / "no_rayleigh.db")
    shutil.copy(DB, path)
    conn = sqlite3.connect(path)
    conn.execute("DROP TABLE rayleigh")
    conn.commit()
    conn.close()
    return path


def _same(opa, expect):
    assert opa.rayleigh_molecules == list(expect) == list(opa.rayleigh_opa) == list(opa._ray)
    for m, v in expect.items():
        assert np.array_equal(opa.rayleigh_opa[m], v) and np.array_equal(opa._ray[m].to_host(), v), m
        assert opa.rayleigh_opa[m].shape == (opa.nwno,)


def test_from_sqlite_rule(px, bare_db, gold):
    from picaso_amd.rayleigh import Rayleigh
    wno = gold["db/wno"]
    ctx = object()
    computed = {m: Rayleigh(wno).compute_sigma(m) for m in gold["molecules"]}
    opa = px.RetrieveOpacities.from_sqlite(bare_db, ctx=ctx)
    assert len(opa.rayleigh_molecules) == 39
    _same(opa, computed)
    _same(px.RetrieveOpacities.from_sqlite(DB, ctx=ctx), _db_rayleigh())          # the table's four, its bits
    for db in (DB, bare_db):
        _same(px.RetrieveOpacities.from_sqlite(db, rayleigh_opa={}, ctx=ctx), {})
        x = 1e-27 * (wno / 1e4) ** 4
        _same(px.RetrieveOpacities.from_sqlite(db, rayleigh_opa={"H2": x}, ctx=ctx), {"H2": x})
    # the plain constructor keeps its default of none
    raw = dict(wno=wno, pt_pairs=[(1, 1.0, 300.0), (2, 10.0, 300.0), (3, 1.0, 600.0), (4, 10.0, 600.0)],
               molecular={"H2O": {i: np.ones(wno.size) for i in (1, 2, 3, 4)}}, continuum={"H2H2": {300.0: np.ones(wno.size)}},
               cia_temps=[300.0], ctx=ctx)
    assert px.RetrieveOpacities(**raw).rayleigh_molecules == []


@pytest.mark.parametrize("kw", [dict(wave_range=[0.5, 1.2]), dict(resample=2), dict(wave_range=[0.45, 2.0], resample=2)])
def test_from_sqlite_reduced_grid(px, bare_db, gold, kw):
    from picaso_amd.rayleigh import Rayleigh
    wno = gold["db/wno"]
    opa = px.RetrieveOpacities.from_sqlite(bare_db, ctx=object(), **kw)
    expect = wno[::kw.get("resample", 1)]
    if "wave_range" in kw:
        wave = 1e4 / expect
        expect = expect[(wave > min(kw["wave_range"])) & (wave < max(kw["wave_range"]))]
    assert 1 < expect.size < wno.size and np.array_equal(opa.wno, expect)
    r = Rayleigh(opa.wno)
    _same(opa, {m: r.compute_sigma(m) for m in r.rayleigh_molecules})
    # ... and the database WITH the table gives the table's rows on that grid, as before
    tab = px.RetrieveOpacities.from_sqlite(DB, ctx=object(), **kw)
    sel = np.isin(wno, expect)
    _same(tab, {m: v[sel] for m, v in _db_rayleigh().items()})


@pytest.mark.parametrize("method", ["preweighted", "resortrebin"])
def test_from_files_rule(px, tmp_path, gold, method, h5py):
    from picaso_amd.rayleigh import Rayleigh
    wno = np.sort(gold["db/wno"])
    ref, dw = tck._refdata(tmp_path, wno)
    cdb = str(tmp_path / "cont.db")
    tck._cont_db_on(cdb, wno)
    tabs = tck._tables(wno.size, 8, seed=5)
    if method == "resortrebin":
        d = tmp_path / "resortrebin"
        d.mkdir()
        for m, a in tabs.items():
            np.save(d / ("%s_1460.npy" % m), a)
        ck = str(d)
    else:
        ck = str(tmp_path / "pm.hdf5")
        tck._write_h5(ck, wno, dw, tabs["H2O"], px.g_w_2gauss(), True)
    kw = dict(method=method, ctx=object(), refdata=ref)
    opa = px.RetrieveCKs.from_files(ck, cdb, **kw)
    assert opa.ngauss == 8 and np.allclose(opa.wno, wno, rtol=1e-15)
    r = Rayleigh(opa.wno)
    assert len(opa.rayleigh_molecules) == 39
    _same(opa, {m: r.compute_sigma(m) for m in r.rayleigh_molecules})
    _same(px.RetrieveCKs.from_files(ck, cdb, rayleigh_opa={}, **kw), {})
    x = 1e-27 * (wno / 1e4) ** 4
    _same(px.RetrieveCKs.from_files(ck, cdb, rayleigh_opa={"H2": x}, **kw), {"H2": x})


def test_opannection_passes_none_through(px, bare_db, monkeypatch):
    """jdi.opannection(filename_db=...) on a database without the table: all 39 species (on the parent: none)."""
    from picaso_amd import _lib
    from picaso_amd import justdoit as jdi
    monkeypatch.setattr(_lib, "context", lambda *a, **k: object())
    monkeypatch.delenv("picaso_refdata", raising=False)
    assert len(jdi.opannection(filename_db=bare_db).rayleigh_molecules) == 39
    assert jdi.opannection(filename_db=DB).rayleigh_molecules == ["H2", "He", "CH4", "H2O"]
    assert jdi.opannection(filename_db=bare_db, rayleigh_opa={}).rayleigh_molecules == []


def test_downstream_takes_the_long_list(px, bare_db, gold):
    """ATMSETUP.get_needed_continuum intersects the profile's columns with the 39 (profile order), and shard_opacity
    slices every species' row."""
    from picaso_amd import justdoit as jdi
    from picaso_amd.atmsetup import ATMSETUP
    opa = px.RetrieveOpacities.from_sqlite(bare_db, ctx=object())
    case = jdi.inputs()
    case.phase_angle(0)
    case.gravity(gravity=float(gold["planes/in/gravity"]))
    prof = {"pressure": gold["planes/in/plevel_bar"], "temperature": gold["planes/in/tlevel"]}
    for k in gold["planes/in/columns"]:
        prof[str(k)] = gold["planes/in/mix/" + str(k)]
    case.atmosphere(df=prof)
    atm = ATMSETUP(case.inputs)
    atm.get_profile()
    atm.get_needed_continuum(opa.rayleigh_molecules, opa.avail_continuum)
    assert atm.rayleigh_molecules == list(gold["planes/rayleigh_molecules"]) and len(atm.rayleigh_molecules) == 10
    sh = px.shard_opacity(opa, 5, 17, object())
    assert sh.rayleigh_molecules == opa.rayleigh_molecules and len(sh._ray) == 39
    for m in opa.rayleigh_molecules:
        assert np.array_equal(sh.rayleigh_opa[m], opa.rayleigh_opa[m][5:17])
        assert np.array_equal(sh._ray[m].to_host(), opa.rayleigh_opa[m][5:17])
