"""``picaso_chem_interp_dev`` (csrc/cheminterp.hip) through ``chemistry.chem_interp_batch``, ``inputs.chemeq_3d`` and
``inputs.premix_3d``.  Yardstick: ``chemistry.interp_numpy``, the body of ``inputs.chem_interp``; fixtures:
tests/golden/chemistry.npz and tests/golden/chemistry/ (tests/golden/make_chemistry.py).

Two criteria, for every tested point:
* the exponent (``log10=True``) equals ``interp_numpy``'s bit for bit, NaNs included;
* the abundance lies within ``4 * np.spacing(10.0**x)`` of numpy's ``10.0**x`` wherever ``x`` is finite and in [-300, 300], and
  is NaN, infinite or zero exactly where numpy's is.  The 4: the device's ``2**y`` (1 ulp), the carried rounding error of
  ``x * log2(10)`` (1 ulp), the final product (0.5 ulp) and glibc's ``pow`` (under 1 ulp); DESIGN 5l.
"""
import ctypes
import os
import shutil

import numpy as np
import pytest

from helpers import GOLDEN
from test_chemistry_host import CHEM_DIR, DIR_2121, ragged_1060, species_of, table_of

pytestmark = pytest.mark.gpu
DB = os.path.join(GOLDEN, "synthetic_opacities.db")
RTOL_REFERENCE = 1e-12          # the abundance against the reference: test_chemistry_host.py (4 ulp is far inside it)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "chemistry.npz"))


@pytest.fixture(scope="module")
def expected():
    return np.load(os.path.join(CHEM_DIR, "expected.npz"))


@pytest.fixture(scope="module")
def tab2121(gold):
    return table_of(gold, "t2121")


def extra_points(tab, n, seed):
    """``n`` points aimed at the kernel's branches: the ragged-edge clamp (P above the third-last pressure of a column), T on
    grid temperatures, P on grid pressures, T = NaN, P = NaN, P = 0, then random ones."""
    temps, press = np.unique(tab["temperature"]), np.unique(tab["pressure"])
    rng = np.random.default_rng(seed)
    t, p = [], []
    for pv in (press[-3], press[-3] * 1.0001, press[-2], press[-2] * 3.0, press[-1], press[-1] * 7.0):      # the clamp
        for tv in (temps[0] * 1.01, temps[len(temps) // 2] * 1.003, temps[-1] * 0.99):
            t.append(tv)
            p.append(pv)
    for tv in temps[::7]:                                              # T exactly on a grid temperature
        t.append(tv)
        p.append(10 ** rng.uniform(np.log10(press[0]), np.log10(press[-1])))
    for pv in press:                                                   # P exactly on a grid pressure
        t.append(rng.uniform(temps[0], temps[-1]))
        p.append(pv)
    mid_t, mid_p = temps[len(temps) // 3] * 1.02, press[len(press) // 2] * 1.5
    t += [np.nan, mid_t, mid_t, np.nan, np.nan]
    p += [mid_p, np.nan, 0.0, np.nan, 0.0]
    k = n - len(t)
    assert k > 0
    t += list(rng.uniform(0.7 * temps[0], 1.2 * temps[-1], k))
    p += list(10 ** rng.uniform(np.log10(press[0]) - 2, np.log10(press[-1]) + 2, k))
    return np.array(t), np.array(p)


@pytest.fixture(scope="module")
def points(tab2121, expected):
    """1 003 points (no multiple of 64 or 256): the fixture's scattered set plus ``extra_points``."""
    t, p = extra_points(tab2121, 503, 11)
    t = np.concatenate([expected["scatter/temperature"], t])
    p = np.concatenate([expected["scatter/pressure"], p])
    assert t.size == 1003
    return t, p


def mirror(t, p, tab):
    """``(species, exponent (npoints, nspecies))`` of the numpy form, computed once per point set."""
    from picaso_amd import chemistry as ch
    with np.errstate(all="ignore"):
        return ch.interp_numpy(t, p, tab, log10=True)


@pytest.fixture(scope="module")
def mirror_1003(points, tab2121):
    return mirror(*points, tab2121)


@pytest.fixture(scope="module")
def device_1003(points, tab2121):
    """The two device results of the 1 003 points, shared by the tests that compare against them."""
    from picaso_amd import chemistry as ch
    t, p = points
    return ch.chem_interp_batch(t, p, tab2121, log10=True), ch.chem_interp_batch(t, p, tab2121)


def check_exponent(got, species, x):
    for i, sp in enumerate(species):
        assert got[sp].shape == x[:, i].shape
        assert np.array_equal(got[sp], x[:, i], equal_nan=True), sp


def check_abundance(got, species, x):
    worst = 0.0
    with np.errstate(all="ignore"):
        ref = 10.0 ** x
    for i, sp in enumerate(species):
        g, r, xi = got[sp], ref[:, i], x[:, i]
        assert np.array_equal(np.isnan(g), np.isnan(r)) and np.array_equal(np.isinf(g), np.isinf(r)), sp
        assert np.array_equal(g == 0, r == 0), sp
        ok = np.isfinite(xi) & (np.abs(xi) <= 300)
        ulps = np.abs(g[ok] - r[ok]) / np.spacing(r[ok])
        worst = max(worst, float(ulps.max()) if ulps.size else 0.0)
    print("abundance: worst distance from numpy's 10.0**x: %.2f ulp" % worst)
    assert worst <= 4.0
    return worst


# ------------------------------------------------------------------------------------------------------ points
def test_1003_points_exponent_is_the_mirrors_bit_for_bit(mirror_1003, device_1003, points):
    species, x = mirror_1003
    assert len(species) == 50 and np.isnan(x).any() and np.isfinite(x).any()
    assert list(device_1003[0]) == species
    check_exponent(device_1003[0], species, x)


def test_1003_points_abundance_within_4_ulp(mirror_1003, device_1003):
    species, x = mirror_1003
    assert np.nanmin(x) < -50 and np.nanmax(x) > 0                    # the range where the plain product fails by > 100 ulp
    check_abundance(device_1003[1], species, x)


def test_ragged_table_257_points(gold, expected):
    from picaso_amd import chemistry as ch
    tab = ragged_1060(gold)
    t, p = extra_points(tab, 257, 5)
    species, x = mirror(t, p, tab)
    nc_p = ch.table_grids(tab)[4]
    assert nc_p.min() == 3 and len(np.unique(nc_p)) > 3
    check_exponent(ch.chem_interp_batch(t, p, tab, log10=True), species, x)
    check_abundance(ch.chem_interp_batch(t, p, tab), species, x)


# ------------------------------------------------------------------------------------------------------ small shapes
def test_one_point_and_one_species(tab2121, mirror_1003, points):
    from picaso_amd import chemistry as ch
    species, x = mirror_1003
    t, p = points
    one = ch.chem_interp_batch(t[7:8], p[7:8], tab2121, log10=True)
    assert all(one[sp].shape == (1,) and one[sp][0] == x[7, i] for i, sp in enumerate(species))
    scalar = ch.chem_interp_batch(t[7], p[7], tab2121, species="H2O", log10=True)
    assert list(scalar) == ["H2O"] and scalar["H2O"].shape == () and scalar["H2O"] == x[7, species.index("H2O")]
    col = ch.chem_interp_batch(t, p, tab2121, species=["CH4"], log10=True)
    assert list(col) == ["CH4"] and np.array_equal(col["CH4"], x[:, species.index("CH4")], equal_nan=True)
    with pytest.raises(KeyError, match="XeF6"):
        ch.chem_interp_batch(t, p, tab2121, species=["H2O", "XeF6"])


def test_zero_points_launch_nothing(tab2121, monkeypatch):
    from picaso_amd import chemistry as ch
    ch.chem_interp_batch(np.ones(1) * 500.0, np.ones(1), tab2121)      # the table is resident from here on

    def no_launch(*a, **k):
        raise AssertionError("zero points must not reach the kernel")
    monkeypatch.setattr(ch, "chem_interp_dev", no_launch)
    out = ch.chem_interp_batch(np.empty((0, 3)), np.empty((0, 3)), tab2121)
    assert len(out) == 50 and all(v.shape == (0, 3) for v in out.values())
    dev, names = ch.chem_interp_batch(np.empty(0), np.empty(0), tab2121, out="device")
    assert dev is None and len(names) == 50


def test_the_c_entry_refuses_bad_arguments_and_takes_zero_points(tab2121):
    from picaso_amd import _lib
    from picaso_amd import chemistry as ch
    tab = ch.ChemTable.resident(tab2121)
    lib, ctx = _lib.load(), tab.ctx
    g, i = tab.d_grids.addr, tab.d_ints.addr

    def call(ntemp=tab.ntemp, npres=tab.npres, npoints=0, nsel=tab.nspecies):
        return lib.picaso_chem_interp_dev(ctx, tab.nrow, tab.nspecies, tab.d_log_abunds.addr, ntemp, npres, g, g + 8 * tab.ntemp, i,
                                          i + 4 * tab.ntemp, npoints, None, None, nsel, None, 0, None)
    assert call() == 0                                                 # zero points: no launch, no pointer is looked at
    for kw, word in ((dict(ntemp=1), "two temperatures"), (dict(npoints=-1), "negative"), (dict(nsel=3), "selection"),
                     (dict(npoints=5), "NULL"), (dict(npres=9000), "LDS")):
        assert call(**kw) != 0
        assert word in lib.picaso_last_error(ctx).decode(), kw


def test_a_shuffled_37_species_subset_equals_the_full_call(tab2121, device_1003, points):
    from picaso_amd import chemistry as ch
    t, p = points
    full_x, full_a = device_1003
    names = list(np.random.default_rng(3).permutation(list(full_x))[:37])
    assert names != [s for s in full_x if s in names]                  # shuffled, not table order
    sub_x = ch.chem_interp_batch(t, p, tab2121, species=names, log10=True)
    sub_a = ch.chem_interp_batch(t, p, tab2121, species=names)
    assert list(sub_x) == names and list(sub_a) == names
    for sp in names:
        assert np.array_equal(sub_x[sp], full_x[sp], equal_nan=True) and np.array_equal(sub_a[sp], full_a[sp], equal_nan=True)


def test_out_device_keeps_the_result_resident(tab2121, device_1003, points):
    from picaso_amd import chemistry as ch
    from picaso_amd.device import DeviceArray
    t, p = points
    dev, names = ch.chem_interp_batch(t.reshape(17, 59), p.reshape(17, 59), tab2121, out="device")
    assert isinstance(dev, DeviceArray) and dev.shape == (50, 1003) and names == list(device_1003[1])
    host = dev.to_host()
    assert all(np.array_equal(host[i], device_1003[1][sp], equal_nan=True) for i, sp in enumerate(names))
    shaped = ch.chem_interp_batch(t.reshape(17, 59), p.reshape(17, 59), tab2121, species=["CO"])
    assert shaped["CO"].shape == (17, 59) and np.array_equal(shaped["CO"].ravel(), device_1003[1]["CO"], equal_nan=True)


def test_a_points_result_does_not_depend_on_its_neighbours(tab2121, device_1003, points):
    from picaso_amd import chemistry as ch
    t, p = points
    rev_x = ch.chem_interp_batch(t[::-1], p[::-1], tab2121, log10=True)
    rev_a = ch.chem_interp_batch(t[::-1], p[::-1], tab2121)
    for sp in device_1003[0]:
        assert np.array_equal(rev_x[sp][::-1], device_1003[0][sp], equal_nan=True), sp
        assert np.array_equal(rev_a[sp][::-1], device_1003[1][sp], equal_nan=True), sp


# ------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("case", ["hj", "scatter"])
def test_against_the_references_abundances(tab2121, expected, case):
    from picaso_amd import chemistry as ch
    t, p = expected[case + "/temperature"], expected[case + "/pressure"]
    got = ch.chem_interp_batch(t, p, tab2121)
    species = species_of(expected, case, "2121")
    assert list(got) == species
    worst = 0.0
    for sp in species:
        want = expected["%s/2121/%s" % (case, sp)]
        assert np.all(np.isfinite(want)) and np.all(want > 0)
        worst = max(worst, float(np.max(np.abs(got[sp] - want) / want)))
    print("%s: worst relative distance from the reference %.2e" % (case, worst))
    assert worst <= RTOL_REFERENCE


# ------------------------------------------------------------------------------------------------------ chemeq_3d, premix_3d
def _mem(ctx):
    from picaso_amd import _lib
    o = (ctypes.c_size_t * 6)()
    _lib.check(_lib.load().picaso_ctx_mem_stats(ctx, o), ctx)
    return int(o[0]), int(o[1])


class _Opa:
    def __init__(self, full_abunds):
        self.full_abunds = full_abunds


def _facet_case(jdi, expected):
    c = jdi.inputs()
    c.phase_angle(0.7, num_gangle=3, num_tangle=2)
    c.atmosphere_3d({"pressure": expected["facets/pressure"], "temperature": expected["facets/temperature"]})
    return c


def test_premix_3d_reproduces_the_reference_column_by_column(tab2121, expected):
    from picaso_amd import chemistry as ch
    from picaso_amd import justdoit as jdi
    c = _facet_case(jdi, expected)
    c.inputs["atmosphere"]["profile_3d"]["H2O"] = np.zeros((12, 3, 2))           # a column that is there is replaced
    c.premix_3d(_Opa(tab2121))
    prof = c.inputs["atmosphere"]["profile_3d"]
    species = species_of(expected, "facets", "2121")
    assert list(prof) == ["pressure", "temperature", "H2O"] + [s for s in species if s != "H2O"]
    t3, p3 = expected["facets/temperature"], np.broadcast_to(expected["facets/pressure"][:, None, None], (12, 3, 2))
    _, x = mirror(t3.ravel(), p3.ravel(), tab2121)
    for i, sp in enumerate(species):
        want = expected["facets/2121/" + sp]
        assert prof[sp].shape == (12, 3, 2) and prof[sp].flags["C_CONTIGUOUS"]
        assert np.max(np.abs(prof[sp] - want) / want) <= RTOL_REFERENCE, sp
        assert np.max(np.abs(prof[sp].ravel() - 10.0 ** x[:, i]) / np.spacing(10.0 ** x[:, i])) <= 4.0, sp
    # a second call finds the table resident: nothing is uploaded, nothing stays behind
    before, mem = ch.UPLOADS, _mem(ch.ChemTable.resident(tab2121).ctx)
    c.premix_3d(_Opa(dict(tab2121)))                                   # another dictionary of the same content
    assert ch.UPLOADS == before and _mem(ch.ChemTable.resident(tab2121).ctx) == mem
    with pytest.raises(Exception, match="full_abunds"):
        c.premix_3d(object())


def test_chemeq_3d_reads_the_grid_under_refdata(gold, tmp_path, monkeypatch):
    """``$picaso_refdata`` points at a directory that holds the cut-down grid: ``chemeq_3d`` chooses the file, reads it once
    and fills every facet; a temperature shared by the facets gives ``(nlevel,)`` columns."""
    from picaso_amd import chemistry as ch
    from picaso_amd import justdoit as jdi
    shutil.copytree(DIR_2121, str(tmp_path / "chemistry" / "visscher_grid_2121"))
    monkeypatch.setenv("picaso_refdata", str(tmp_path))
    cut = table_of(gold, "cut2121")
    temps = np.unique(cut["temperature"])
    rng = np.random.default_rng(9)
    p = np.logspace(-6, 2, 7)
    t3 = rng.uniform(temps[0] * 0.9, temps[1] * 1.1, (7, 3, 2))
    c = jdi.inputs()
    c.phase_angle(0.7, num_gangle=3, num_tangle=2)
    c.atmosphere_3d({"pressure": p, "temperature": t3})
    reads = []
    real = ch.read_visscher_2121
    monkeypatch.setattr(ch, "read_visscher_2121", lambda f: (reads.append(os.path.basename(f)), real(f))[1])
    c.chemeq_3d(log_mh=0.1, cto_absolute=0.6, n_cpu=4)
    assert reads == ["sonora_2121grid_feh0.0_co0.55.txt"]
    prof = c.inputs["atmosphere"]["profile_3d"]
    species, x = mirror(t3.ravel(), np.broadcast_to(p[:, None, None], t3.shape).ravel(), cut)
    for i, sp in enumerate(species):
        assert prof[sp].shape == (7, 3, 2)
        assert np.max(np.abs(prof[sp].ravel() - 10.0 ** x[:, i]) / np.spacing(10.0 ** x[:, i])) <= 4.0, sp
    uploads, first = ch.UPLOADS, {sp: prof[sp].copy() for sp in species}
    with pytest.warns(UserWarning, match="cto_absolute"):
        c.chemeq_3d(c_o=1.0)                                           # 0.55 * 1.0: the same file
    assert reads == ["sonora_2121grid_feh0.0_co0.55.txt"] * 2
    assert ch.UPLOADS == uploads                                       # read again, found resident by its content
    assert all(np.array_equal(prof[sp], first[sp]) for sp in species)
    shared = jdi.inputs()
    shared.phase_angle(0.7, num_gangle=3, num_tangle=2)
    shared.atmosphere_3d({"pressure": p, "temperature": t3[:, 1, 1]})
    shared.chemeq_3d()
    prof1 = shared.inputs["atmosphere"]["profile_3d"]
    assert all(prof1[sp].shape == (7,) and np.array_equal(prof1[sp], prof[sp][:, 1, 1]) for sp in species)


def test_two_phases_of_profile_4d_give_what_profile_3d_gives_alone(tab2121, expected):
    from picaso_amd import justdoit as jdi
    t3, p = expected["facets/temperature"], expected["facets/pressure"]
    phases = [{"pressure": p, "temperature": t3}, {"pressure": p, "temperature": t3[::-1] * 1.07}]
    alone = []
    for ph in phases:
        c = jdi.inputs()
        c.phase_angle(0.7, num_gangle=3, num_tangle=2)
        c.atmosphere_3d(ph)
        c.premix_3d(_Opa(tab2121))
        alone.append(c.inputs["atmosphere"]["profile_3d"])
    c = jdi.inputs()
    c.phase_curve_geometry("thermal", [0.0, 1.5], num_gangle=3, num_tangle=2)
    c.atmosphere_4d(phases)
    c.premix_3d(_Opa(tab2121))
    both = c.inputs["atmosphere"]["profile_4d"]
    assert len(both) == 2
    for got, want in zip(both, alone):
        assert list(got) == list(want) and len(got) == 52
        assert all(np.array_equal(got[k], want[k]) for k in want)


# ------------------------------------------------------------------------------------------------------ end to end
def test_spectrum_3d_after_chemeq_3d_against_the_spectrum_of_the_mirrors_columns(tab2121, monkeypatch):
    """``atmosphere_3d(profiles without chemistry)``, ``chemeq_3d`` (handed the full 2121 table in place of the file under
    ``$picaso_refdata``), ``spectrum(dimension='3d')`` on the small 3-D scene of tests/test_convolve_gpu.py, against the
    spectrum of a case that is handed abundances as columns.

    Two comparisons.  Handed the columns ``chemeq_3d`` stored, the spectrum is the same bit for bit: the call adds columns
    and nothing else.  Handed ``interp_numpy``'s columns it cannot be: the device's ``10**x`` is held to 4 ulp of numpy's,
    not to its bits (glibc's ``pow`` is not correctly rounded either, so no device function could promise them), and a
    spectrum of columns that differ in their last bits differs in its last bits.  What is asserted there is ``RTOL_SPECTRUM``
    = 1e-10: every abundance moves by at most 4 * 2^-52 = 9e-16 relative, optical depths (sums of positive terms) by the same,
    and the solver amplifies a last-bit change of its inputs by far less than the five orders left (the suite holds kernels
    that differ from the oracle in last bits inside the solver to 1e-8); a wrong cell, row or species moves an abundance by
    percents.  The count of spectral points that do differ from the numpy-column spectrum is printed."""
    from picaso_amd import chemistry as ch
    from picaso_amd import justdoit as jdi
    RTOL_SPECTRUM = 1e-10
    og = np.load(os.path.join(GOLDEN, "optics.npz"))
    opa = jdi.opannection(filename_db=DB, query_method="linear")
    p = og["in/plevel_bar"]
    t3 = og["in/tlevel"][:, None, None] * (1.0 + 0.02 * np.arange(6).reshape(1, 3, 2))
    keys = ("albedo", "thermal", "fpfs_reflected", "fpfs_thermal")

    def scene(profile):
        c = jdi.inputs()
        c.phase_angle(0.7, num_gangle=3, num_tangle=2)
        c.gravity(gravity=float(og["in/gravity"]), radius=7.1e9, mass=1.9e30)
        c.atmosphere_3d(profile)
        c.star(relative_flux=1.0 + 0.3 * np.sin(np.arange(opa.nwno) / 7.0), radius=6.9e10, semi_major=7.5e12)
        c.approx(raman="none")
        return c

    def spectrum(c):
        return c.spectrum(opa, dimension="3d", calculation="reflected+thermal")
    monkeypatch.setattr(ch, "visscher_2121", lambda cto_absolute, log_mh, directory=None: tab2121)
    a = scene({"pressure": p, "temperature": t3})
    a.chemeq_3d()
    prof = a.inputs["atmosphere"]["profile_3d"]
    assert len(prof) == 52 and prof["H2"].shape == t3.shape and 0.5 < prof["H2"].min() < 1.0
    out_a = spectrum(a)
    out_b = spectrum(scene({k: np.array(v) for k, v in prof.items()}))
    for k in keys:
        assert np.all(np.isfinite(out_a[k])) and np.array_equal(out_a[k], out_b[k]), k
    species, x = mirror(t3.ravel(), np.broadcast_to(p[:, None, None], t3.shape).ravel(), tab2121)
    cols = {"pressure": p, "temperature": t3}
    cols.update({sp: (10.0 ** x[:, i]).reshape(t3.shape) for i, sp in enumerate(species)})
    assert list(cols) == list(prof)
    out_n = spectrum(scene(cols))
    for k in keys:
        rel = np.abs(out_a[k] - out_n[k]) / np.abs(out_n[k])
        print("%s: %d of %d points differ from the numpy-column spectrum, worst relative distance %.2e"
              % (k, int(np.count_nonzero(out_a[k] != out_n[k])), rel.size, float(rel.max())))
        assert rel.max() <= RTOL_SPECTRUM, k
    # the chemistry matters to this spectrum: H2O alone moves it
    wet = scene(dict({k: np.array(v) for k, v in prof.items()}, H2O=prof["H2O"] * 3.0))
    assert not np.array_equal(spectrum(wet)["albedo"], out_a["albedo"])
