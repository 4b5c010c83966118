"""The opacity-database factory on the device (csrc/contfactory.hip through picaso_amd/opacity_factory.py): ``continuum_rows``
against what the reference produced (tests/golden/continuum_factory.npz) within the bounds of DESIGN section 5q, the median
filter against ``scipy.signal.medfilt`` of the device's own unfiltered row on both selection paths, ``insert_molecular_1460``
against the reference's rows bit for bit, and a database built end to end against an opacity object made from arrays."""
import warnings

import numpy as np
import pytest

import continuum_factory_cases as cc
from picaso_amd import _lib
from picaso_amd import justdoit as jdi
from picaso_amd import opacity_factory as of
from picaso_amd import optics
from picaso_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

TEMPS = cc.fixture()["temperatures"]


def host_rows(g, smooth=True):
    table, nsp = cc.RUNS[g]
    old_wno, og = cc.cia(table)
    ov, bell = cc.tables()
    rows = of.continuum_rows_numpy(og, TEMPS, old_wno, cc.MOLECULES, cc.grid(g), ov, bell, smooth=smooth)
    if smooth:
        assert np.array_equal(cc.bits(rows[:, :nsp]), cc.bits(cc.fixture()["rows/" + g]))
    return rows


def device_rows(g, **kw):
    old_wno, og = cc.cia(cc.RUNS[g][0])
    ov, bell = cc.tables()
    return of.continuum_rows(og, TEMPS, old_wno, cc.MOLECULES, cc.grid(g), ov, bell, **kw)


def h2h2_classes(g, i):
    """Masks over the grid for temperature ``i``: ``(exact, linsky_exp, linsky_low)``: points whose H2H2 value has no
    transcendental on the device (the placeholder itself, Linsky's rational branch), the points of Linsky's exp branch, and
    whether a Linsky point lies below 12000 cm-1 (the row is smoothed)."""
    old_wno, og = cc.cia(cc.RUNS[g][0])
    ov, _ = cc.tables()
    w, t = cc.grid(g), TEMPS[i]
    v = 10 ** np.interp(w, old_wno, og[i, 0], left=-33, right=-33)
    h, loc, add = of.h2h2_overtone(t, w, ov)
    if add:
        v[loc] = h
    lin = (v == 1e-33) & (w >= 1000)
    w0, d = of._linsky_params(t)[:2]
    low = w < w0 + 1.5 * d
    return (lin & low) | ((v == 1e-33) & ~lin), lin & ~low, bool(np.any(lin & (w < 12000)))


def region(g):
    w = cc.grid(g)
    return np.where((w > 9950) & (w < 11200))[0]


@pytest.mark.parametrize("g", sorted(cc.RUNS))
def test_rows_against_the_reference(g):
    """The bounds are DESIGN section 5q's, in ulp of the reference value.  Measured on an MI355X, the maximum over the six
    grids: 10**x rows 1 (bound 4), Linsky's exp branch 2 (bound 8), H-bf 3 (bound 8); H2-, H-ff, the constant rows, the
    placeholders and Linsky's rational branch are equal bit for bit."""
    want, plain = host_rows(g), host_rows(g, smooth=False)
    got, got_plain = device_rows(g), device_rows(g, smooth=False)
    w, reg = cc.grid(g), region(g)
    assert got.shape == want.shape == (9, 5, w.size)
    worst = {"exp10": 0.0, "linsky": 0.0, "hbf": 0.0}
    for i, t in enumerate(TEMPS):
        exact, lin_exp, low = h2h2_classes(g, i)
        # H2H2 before the filter
        u = cc.ulps(got_plain[i, 0], plain[i, 0])
        assert np.array_equal(cc.bits(got_plain[i, 0][exact]), cc.bits(plain[i, 0][exact])), t
        assert np.all(u[lin_exp] <= cc.ULP_LINSKY) and np.all(u[~lin_exp] <= cc.ULP_EXP10), (t, u.max())
        worst["linsky"] = max(worst["linsky"], float(u[lin_exp].max(initial=0.0)))
        worst["exp10"] = max(worst["exp10"], float(u[~lin_exp].max(initial=0.0)))
        # H2H2 after it: outside the region nothing moved; inside, an order statistic of values within the row's bounds
        outside = np.ones(w.size, dtype=bool)
        if low:
            outside[reg] = False
            zero = want[i, 0][reg] == 0.0
            assert np.array_equal(got[i, 0][reg][zero], want[i, 0][reg][zero])
            assert np.all(cc.ulps(got[i, 0][reg], want[i, 0][reg]) <= cc.ULP_LINSKY), t
        assert np.array_equal(cc.bits(got[i, 0][outside]), cc.bits(got_plain[i, 0][outside])), t
        # H2He
        u = cc.ulps(got[i, 1], want[i, 1])
        placeholder = want[i, 1] == 1e-33
        assert np.all(u <= cc.ULP_EXP10) and np.array_equal(got[i, 1][placeholder], want[i, 1][placeholder]), (t, u.max())
        worst["exp10"] = max(worst["exp10"], float(u.max()))
        # H2-, H-ff: bit for bit; H-bf: bounded, its constant parts equal
        assert np.array_equal(cc.bits(got[i, 2]), cc.bits(want[i, 2])), t
        assert np.array_equal(cc.bits(got[i, 4]), cc.bits(want[i, 4])), t
        u = cc.ulps(got[i, 3], want[i, 3])
        const = want[i, 3] == 1e-33
        assert np.all(u <= cc.ULP_HBF) and np.array_equal(got[i, 3][const], want[i, 3][const]), (t, u.max())
        worst["hbf"] = max(worst["hbf"], float(u.max()))
        if t < 600:
            assert np.all(got[i, 2] == 1e-33)
        if t < 800:
            assert np.all(got[i, 3] == 1e-33) and np.all(got[i, 4] == 1e-33 * 1e-30)
    print("grid %s: worst ulp %s" % (g, worst))


@pytest.mark.parametrize("g,cap", [("a", 0), ("b", 0), ("b", 4), ("c", 0), ("c", 64), ("e", 0), ("f", 0), ("d", 0)])
def test_median_filter_is_exact_on_both_paths(g, cap):
    sig = pytest.importorskip("scipy.signal")
    w, reg = cc.grid(g), region(g)
    window = of.smoothing_window(w)
    assert (g, window, reg.size) in (("a", 51, 20), ("b", 7, 89), ("c", 101, 1389), ("d", 7, 89), ("e", 3, 0), ("f", 1, 1))
    plain, got = device_rows(g, smooth=False), device_rows(g, _lds_cap=cap)
    flagged = 0
    for i, t in enumerate(TEMPS):
        low = h2h2_classes(g, i)[2]
        want = plain[i].copy()
        if low and reg.size:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                want[0][reg] = sig.medfilt(plain[i, 0][reg], kernel_size=window)
            flagged += 1
        assert np.array_equal(cc.bits(got[i]), cc.bits(want)), t
    assert flagged == (0 if g in ("d", "e") else 9)
    if g == "a":
        assert np.all(got[:, 0][:, reg] == 0.0)                       # the window is longer than the region: zeros


def test_rows_do_not_depend_on_the_chunk(tmp_path):
    """The database writer: chunks of one temperature, two in flight, against one launch for all."""
    ov, bell = cc.tables()
    whole = device_rows("b")
    db = str(tmp_path / "dev.db")
    of.build_skeleton(db)
    w = cc.grid("b")
    of.restruct_continuum(cc.write_cia(tmp_path / "cia.txt", "gaps"), cc.COLNAMES, w, db, budget_bytes=8 * 5 * w.size,
                          overtone_table=ov, h2minus_table=bell)
    cur, conn = of.open_local(db)
    of.insert_wno_grid(w, cur, conn)
    wno, continuum, cia_temps = optics.read_continuum_db(db)
    assert np.array_equal(wno, w) and np.array_equal(cia_temps, TEMPS)
    for k, name in enumerate(cc.SPECIES):
        for i, t in enumerate(TEMPS):
            assert np.array_equal(cc.bits(continuum[name][float(t)]), cc.bits(whole[i, k])), (name, t)
    with pytest.raises(Exception, match="already holds continuum rows"):
        of.restruct_continuum(str(tmp_path / "cia.txt"), cc.COLNAMES, w, db, overtone_table=ov, h2minus_table=bell)


def test_entry_point_refusals():
    lib, ctx = _lib.load(), _lib.context()
    d = DeviceArray((64,), ctx)
    a = d.addr
    base = [ctx, 1, 2, 0, 4, a, a, 4, a, 2, a, a, 2, a, a, a, 0, 0, 1, 0, 1, a, a]
    for pos, value, msg in ((18, 2, "window must be odd"), (16, 5, "smoothing region"), (17, 5, "smoothing region"),
                            (3, 2, "h2h2 must be"), (1, 0, "ntemp must be"), (19, 8193, "lds_cap must be"),
                            (5, None, "required array argument is NULL")):
        args = list(base)
        args[pos] = value
        assert lib.picaso_continuum_rows_dev(*args) != 0
        assert msg in lib.picaso_last_error(ctx).decode(), msg
    assert lib.picaso_xsec_resample_dev(ctx, 4, a, a, 1, a, a, 0.0, 0.0, 1e-100, 1e-100, 1e-100) != 0
    assert "at least 2 knots" in lib.picaso_last_error(ctx).decode()
    with pytest.raises(Exception, match="must be neighbours on the device route"):
        old_wno, og = cc.cia("gaps")
        ov, bell = cc.tables()
        of.continuum_rows(og, TEMPS, old_wno, cc.MOLECULES, np.array([10000.0, 500.0, 10100.0]), ov, bell)
    d.free()


@pytest.mark.parametrize("form", ["npy", "p_"])
@pytest.mark.parametrize("mode", ["new_R", "new_dwno"])
def test_resampled_rows_equal_the_reference(tmp_path, form, mode):
    f = cc.fixture()
    root = cc.write_xsec(tmp_path / "xsec", form)
    db = str(tmp_path / "m.db")
    of.build_skeleton(db)
    lo, hi = cc.gen.MOL_RANGE
    grid = of.insert_molecular_1460("H2O", lo, hi, root, db, **cc.gen.MOL_MODES[mode])
    assert np.array_equal(cc.bits(grid), cc.bits(f["mol/%s/grid" % mode]))
    opa = of.get_molecular(db, ["H2O"], [300.0, 300.0, 900.0], [1e-3, 1.0, 1.0])
    assert np.array_equal(opa["wavenumber"], grid)
    d = of._Directory("test", root)
    for k, (t, p) in enumerate(((300.0, 1e-3), (300.0, 1.0), (900.0, 1.0))):
        got = opa["H2O"][t][p]
        assert np.array_equal(cc.bits(got), cc.bits(f["mol/%s/row%d" % (mode, k + 1)])), k         # the reference's rows
        restated = of.resample_numpy(f["mol/rows"][k], d.grid_of(k + 1), grid)
        assert np.array_equal(cc.bits(got), cc.bits(restated)), k
    assert np.any(opa["H2O"][900.0][1.0][:3] == 1e-100) and np.any(opa["H2O"][900.0][1.0][-3:] == 1e-100)   # the fills


def test_unresampled_grid_equals_get_wvno_grid(tmp_path):
    root = cc.write_xsec(tmp_path / "xsec", "npy")
    db = str(tmp_path / "m.db")
    of.build_skeleton(db)
    grid = of.insert_molecular_1460("H2O", 2.3, 4.9, root, db, new_R=3000, old_R=3000)
    assert np.array_equal(grid, of.get_wvno_grid(None, 2.3, 4.9, 3000)[2])
    cur, conn = of.open_local(db)
    cur.execute("SELECT wavenumber_grid FROM header")
    assert np.array_equal(cur.fetchone()[0], grid)
    conn.close()


def test_database_end_to_end(tmp_path):
    """A database from the synthetic directory and CIA file, opened by ``opannection`` and run through a 10-layer thermal
    spectrum, against an opacity object made from arrays: the reference's molecular rows and the host's continuum rows.

    The bound.  The molecular rows are equal bit for bit; a continuum row differs by at most 8 ulp <= 16 u, u = 2^-53, so a
    layer's optical depth x moves by at most 16 u x.  Every factor of the flux that depends on a layer is exp(-x / mu) or
    (1 - exp(-x / mu)) times the layer's source: its relative change is at most 16 u x / mu, and a layer with x / mu > 40 is
    invisible behind exp(-40).  Two such factors per layer, 10 layers, and a factor 16 for the conditioning of the
    two-stream solve: 16 u * 40 * 2 * 10 * 16 = 2.3e-11 relative.  Measured on an MI355X: 1.5e-15."""
    f = cc.fixture()
    ov, bell = cc.tables()
    root = cc.write_xsec(tmp_path / "xsec", "npy")
    db = str(tmp_path / "opacities.db")
    of.build_skeleton(db)
    lo, hi = cc.gen.MOL_RANGE
    grid = of.insert_molecular_1460("H2O", lo, hi, root, db, **cc.gen.MOL_MODES["new_R"])
    of.restruct_continuum(cc.write_cia(tmp_path / "cia.txt", "gaps"), cc.COLNAMES, grid, db, overtone_table=ov,
                          h2minus_table=bell)
    opa = jdi.opannection(filename_db=db)
    assert np.array_equal(opa.wno, grid) and list(opa.molecules) == ["H2O"]
    assert opa.avail_continuum == sorted(cc.SPECIES)
    stored = optics.read_continuum_db(db)[1]                          # from_sqlite holds the database's bits
    for name in cc.SPECIES:
        assert np.array_equal(cc.bits(opa._cia[name].to_host()), cc.bits(np.stack([stored[name][float(t)] for t in TEMPS])))
    for k in range(3):
        assert np.array_equal(cc.bits(opa._mol_raw["H2O"].to_host()[k]), cc.bits(f["mol/new_R/row%d" % (k + 1)]))
    old_wno, og = cc.cia("gaps")
    rows = of.continuum_rows_numpy(og, TEMPS, old_wno, cc.MOLECULES, grid, ov, bell)
    molecular = {"H2O": {k + 1: f["mol/new_R/row%d" % (k + 1)] for k in range(3)}}
    continuum = {name: {float(t): rows[i, k] for i, t in enumerate(TEMPS)} for k, name in enumerate(cc.SPECIES)}
    ref = optics.RetrieveOpacities(grid, [(1, 1e-3, 300.0), (2, 1.0, 300.0), (3, 1.0, 900.0)], molecular, continuum, TEMPS,
                                   rayleigh_opa=opa.rayleigh_opa)

    def thermal(o):
        case = jdi.inputs()
        case.phase_angle(0)
        case.gravity(gravity=2500.0)                    # cm/s^2
        case.approx(raman="none")
        p = np.logspace(-4, 1, 11)
        case.atmosphere(df={"pressure": p, "temperature": 700.0 * (p / 0.1) ** 0.1, "H2": np.full(11, 0.84),
                            "He": np.full(11, 0.1599), "H2O": np.full(11, 1e-4)})
        return case.spectrum(o, calculation="thermal")["thermal"]

    got, want = thermal(opa), thermal(ref)
    assert got.shape == grid.shape and np.all(np.isfinite(want)) and np.all(want > 0)
    rel = np.abs(got - want) / want
    bound = 16 * cc.U * 40 * 2 * 10 * 16
    print("end to end: worst relative difference %.3g, bound %.3g" % (rel.max(), bound))
    assert np.all(rel <= bound)
