"""The opacity-database factory on the host (picaso_amd/opacity_factory.py): the continuum sources and
``continuum_rows_numpy`` against what the reference's own functions produced (tests/golden/continuum_factory.npz) bit for
bit, the sqlite schema through the package's readers, chunking, ``overwrite``, the host-only ``insert_direct`` mode and the
refusals."""
import ctypes
import os
import sqlite3

import numpy as np
import pytest

import continuum_factory_cases as cc
from picaso_amd import _lib
from picaso_amd import justdoit as jdi
from picaso_amd import opacity_factory as of
from picaso_amd import optics


def test_the_entry_points_are_declared_and_reexported():
    protos = _lib.declared_prototypes()
    I, L, D, P = ctypes.c_int, ctypes.c_long, ctypes.c_double, ctypes.c_void_p
    assert protos["picaso_continuum_npar"] == (I, [])
    assert protos["picaso_continuum_rows_dev"] == (I, [P, I, I, I, L, P, P, L, P, I, P, P, I, P, P, P, L, L, L, L, I, P, P])
    assert protos["picaso_xsec_resample_dev"] == (I, [P, L, P, P, L, P, P, D, D, D, D, D])
    for name in ("open_local", "build_skeleton", "insert_wno_grid", "continuum_avail", "molecular_avail", "get_continuum",
                 "get_molecular", "delete_molecule", "create_grid_minR", "create_grid", "restruct_continuum",
                 "restructure_opacity", "continuum_rows", "continuum_rows_numpy", "insert_molecular_1460",
                 "insert_hitran_cia"):
        assert callable(getattr(jdi, name)), name


@pytest.mark.parametrize("g", sorted(cc.RUNS))
def test_host_rows_equal_the_reference_bit_for_bit(g):
    table, nsp = cc.RUNS[g]
    old_wno, og = cc.cia(table)
    f = cc.fixture()
    ov, bell = cc.tables()
    got = of.continuum_rows_numpy(og, f["temperatures"], old_wno, cc.MOLECULES, cc.grid(g), ov, bell)
    want = f["rows/" + g]
    assert got.shape == (9, 5, cc.grid(g).size) and want.shape == (9, nsp, cc.grid(g).size)
    assert np.array_equal(cc.bits(got[:, :nsp]), cc.bits(want))


def test_source_functions_equal_the_reference_bit_for_bit():
    f = cc.fixture()
    ov, bell = cc.tables()
    w = cc.grid("a")
    for T in (300.0, 800.0, 2500.0):
        t = np.float64(T)
        h, loc, add = of.h2h2_overtone(t, w, ov)
        assert add == (T <= 350)
        if add:
            assert np.array_equal(cc.bits(h), cc.bits(f["src/overtone/%d" % T])) and np.array_equal(loc[0], f["src/overtone_loc/%d" % T])
        assert np.array_equal(cc.bits(of.fit_linsky(t, w)), cc.bits(f["src/linsky/%d" % T]))
        assert np.array_equal(cc.bits(of.get_h2minus(t, w, bell)), cc.bits(f["src/h2minus/%d" % T]))
        assert np.array_equal(cc.bits(of.get_hminusff(t, w)), cc.bits(f["src/hminusff/%d" % T]))
    assert np.array_equal(cc.bits(of.get_hminusbf(w)), cc.bits(f["src/hminusbf/0"]))
    assert np.all(f["src/hminusff/300"] == 1e-60) and np.any(f["src/hminusff/2500"] == 0.0)


def test_get_original_data_reads_the_cia_file(tmp_path):
    path = cc.write_cia(tmp_path / "cia.txt", "gaps")
    og, temps, old_wno, molecules = of.get_original_data(path, cc.COLNAMES, str(tmp_path / "none.db"))
    want_wno, want = cc.cia("gaps")
    assert molecules == cc.MOLECULES and np.array_equal(temps, cc.fixture()["temperatures"]) and np.array_equal(old_wno, want_wno)
    for k, m in enumerate(molecules):
        assert np.array_equal(og[m].reshape(9, -1), want[:, k])
    assert np.array_equal(og["wno"], np.tile(want_wno, 9))


def test_medfilt_is_scipys():
    sig = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(3)
    for n, k in ((1, 1), (5, 3), (20, 51), (89, 7), (300, 101), (64, 63), (2, 5)):
        x = 10.0 ** rng.uniform(-12, -3, n)
        x[rng.uniform(size=n) < 0.2] = x[0]                # ties
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = sig.medfilt(x, kernel_size=k)
        assert np.array_equal(cc.bits(of.medfilt(x, k)), cc.bits(want)), (n, k)


def _build(tmp_path, name, new_wno, **kw):
    db = str(tmp_path / name)
    of.build_skeleton(db)
    ov, bell = cc.tables()
    of.restruct_continuum(cc.write_cia(tmp_path / (name + ".txt"), "gaps"), cc.COLNAMES, new_wno, db, rows="numpy",
                          overtone_table=ov, h2minus_table=bell, **kw)
    cur, conn = of.open_local(db)
    of.insert_wno_grid(new_wno, cur, conn)
    return db


def _dump(db):
    conn = sqlite3.connect(db)
    rows = conn.execute("SELECT id, molecule, temperature, opacity FROM continuum ORDER BY id").fetchall()
    conn.close()
    return rows


def test_database_is_read_back_by_the_package_readers(tmp_path):
    f = cc.fixture()
    db = _build(tmp_path, "b.db", cc.grid("b"))
    wno, continuum, cia_temps = optics.read_continuum_db(db)
    assert np.array_equal(wno, cc.grid("b")) and np.array_equal(cia_temps, f["temperatures"])
    assert sorted(continuum) == sorted(cc.SPECIES)
    for k, name in enumerate(cc.SPECIES):
        for i, t in enumerate(f["temperatures"]):
            assert np.array_equal(cc.bits(continuum[name][float(t)]), cc.bits(f["rows/b"][i, k])), (name, t)
    assert [r[1] for r in _dump(db)] == cc.SPECIES * 9                 # the reference's insertion order
    molecules, temps = of.continuum_avail(db)
    assert molecules == sorted(cc.SPECIES) and np.array_equal(temps, f["temperatures"])
    got = of.get_continuum(db, ["H2H2", "H-ff"], [310.0, 2400.0])
    assert sorted(got["H2H2"]) == [300.0, 2500.0] and np.array_equal(got["wavenumber"], cc.grid("b"))
    assert np.array_equal(cc.bits(got["H-ff"][2500.0]), cc.bits(f["rows/b"][8, 4]))
    with pytest.raises(Exception, match="Make Temperature a list"):
        of.get_continuum(db, ["H2H2"], 300.0)


def test_grid_of_the_database_equals_get_wvno_grid(tmp_path):
    new_wno = of.get_wvno_grid(None, 0.9, 5.0, 300)[2]
    db = _build(tmp_path, "r.db", new_wno)
    assert np.array_equal(optics.read_continuum_db(db)[0], of.get_wvno_grid(None, 0.9, 5.0, 300)[2])
    assert np.array_equal(new_wno, jdi.create_grid(0.9, 5.0, 300))
    g, dw = of.create_grid_minR(0.9, 5.0, 300)
    assert g[0] == 1e4 / 5.0 and np.all(np.diff(g) > 0) and dw == 1e4 / 0.9 ** 2 * (0.9 / 300) and g[-1] < 1e4 / 0.9


def test_a_budget_of_one_temperature_gives_the_same_file(tmp_path):
    whole = _build(tmp_path, "whole.db", cc.grid("e"))
    nbytes = 8 * 5 * cc.grid("e").size
    single = _build(tmp_path, "single.db", cc.grid("e"), budget_bytes=nbytes)
    tiny = _build(tmp_path, "tiny.db", cc.grid("e"), budget_bytes=1)
    a = _dump(whole)
    assert len(a) == 45 and a == _dump(single) == _dump(tiny)
    with open(whole, "rb") as x, open(single, "rb") as y:
        assert x.read() == y.read()


def test_overwrite(tmp_path):
    db = _build(tmp_path, "o.db", cc.grid("f"))
    ov, bell = cc.tables()
    cia = str(tmp_path / "o.db.txt")
    kw = dict(rows="numpy", overtone_table=ov, h2minus_table=bell)
    with pytest.raises(Exception, match="already holds continuum rows; overwrite=True"):
        of.restruct_continuum(cia, cc.COLNAMES, cc.grid("f"), db, **kw)
    before = _dump(db)
    of.restruct_continuum(cia, cc.COLNAMES, cc.grid("f"), db, overwrite=True, **kw)
    after = _dump(db)
    assert len(after) == 45 and [r[1:] for r in after] == [r[1:] for r in before]
    bare = str(tmp_path / "bare.db")
    with pytest.raises(Exception, match="no continuum table; run build_skeleton"):
        of.restruct_continuum(cia, cc.COLNAMES, cc.grid("f"), bare, **kw)


@pytest.mark.parametrize("form", ["npy", "p_"])
def test_insert_direct_equals_the_reference(tmp_path, form):
    f = cc.fixture()
    root = cc.write_xsec(tmp_path / "xsec", form)
    db = str(tmp_path / "m.db")
    of.build_skeleton(db)
    grid = of.insert_molecular_1460("H2O", cc.gen.MOL_RANGE[0], cc.gen.MOL_RANGE[1], root, db, insert_direct=True)
    assert np.array_equal(grid, f["mol/insert_direct/grid"])
    molecules, pt_pairs = of.molecular_avail(db)
    assert molecules == ["H2O"] and pt_pairs == [(1, 1e-3, 300.0), (2, 1.0, 300.0), (3, 1.0, 900.0)]
    got = of.get_molecular(db, ["H2O"], [310.0, 880.0], [0.9, 1.2])
    assert np.array_equal(cc.bits(got["H2O"][300.0][1.0]), cc.bits(f["mol/insert_direct/row2"]))
    assert np.array_equal(cc.bits(got["H2O"][900.0][1.0]), cc.bits(f["mol/insert_direct/row3"]))
    assert np.array_equal(got["wavenumber"], grid)
    of.delete_molecule("H2O", db)
    assert of.molecular_avail(db) == ([], [])


def test_refusals(tmp_path):
    root = cc.write_xsec(tmp_path / "xsec", "npy")
    db = str(tmp_path / "m.db")
    of.build_skeleton(db)
    args = (2.3, 4.9, root, db)
    with pytest.raises(NotImplementedError, match="insert_hitran_cia: HITRAN's .cia reader is not supported"):
        of.insert_hitran_cia("x.cia", "H2H2", db, cc.grid("f"))
    with pytest.raises(NotImplementedError, match="insert_molecular_1460: the alkali csv form .molecule 'Na'. is not supported"):
        of.insert_molecular_1460("Na", *args, new_R=100)
    with pytest.raises(NotImplementedError, match="insert_molecular_1460: dir_kark_ch4 .* is not supported"):
        of.insert_molecular_1460("H2O", *args, new_R=100, dir_kark_ch4="kark")
    with pytest.raises(NotImplementedError, match="insert_molecular_1460: dir_optical_o3 .* is not supported"):
        of.insert_molecular_1460("H2O", *args, new_R=100, dir_optical_o3="o3")
    os.makedirs(os.path.join(root, "CO"))
    open(os.path.join(root, "CO", "wavelengths.txt"), "w").close()
    with pytest.raises(NotImplementedError, match="insert_molecular_1460: the Lupu text form"):
        of.insert_molecular_1460("CO", *args, new_R=100)
    os.makedirs(os.path.join(root, "NH3"))
    open(os.path.join(root, "NH3", "readomni.fits"), "w").close()
    with pytest.raises(NotImplementedError, match="insert_molecular_1460: the FITS side-file readomni.fits"):
        of.insert_molecular_1460("NH3", *args, new_R=100)
    os.makedirs(os.path.join(root, "PH3"))
    open(os.path.join(root, "PH3", "fort.1"), "w").close()
    with pytest.raises(NotImplementedError, match="insert_molecular_1460: the fort.. text rows"):
        of.insert_molecular_1460("PH3", *args, new_R=100)
    open(os.path.join(root, "TiO.h5"), "w").close()
    with pytest.raises(NotImplementedError, match="insert_molecular_1460: the HDF5 / h5 input form"):
        of.insert_molecular_1460("TiO", *args, new_R=100)
    with pytest.raises(Exception, match="Need to either input a new constant R"):
        of.insert_molecular_1460("H2O", *args)
    ov, bell = cc.tables()
    old_wno, og = cc.cia("gaps")
    with pytest.raises(Exception, match="og_log_opacity must be .ntemp, nmolecules, nold."):
        of.continuum_rows_numpy(og[:, :1], cc.fixture()["temperatures"], old_wno, cc.MOLECULES, cc.grid("f"), ov, bell)
    with pytest.raises(Exception, match="at least 2 points"):
        of.continuum_rows_numpy(og, cc.fixture()["temperatures"], old_wno, cc.MOLECULES, np.array([5000.0]), ov, bell)
