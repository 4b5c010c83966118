"""jdi.thermal_contribution / jdi.transmission_contribution on the GPU (csrc/contribfn.hip) against tests/golden/contribfn.npz
(the reference's justplotit.thermal_contribution / transmission_contribution and a np.longdouble restatement,
tests/golden/make_contribfn.py), against numpy on synthetic planes, and against the difference of two transit depths.

Bounds.  Thermal: 2e-13 relative where |ref| >= 1e-290 -- the Planck routine's 1e-13 (tests/test_planck.py), the device
exp's 2 ulp on an argument with numpy's bits, three roundings.  Transmission: 4 nlevel 745 2^-53 relative where
CF_x80 >= 1e-280 -- the argument of exp carries up to nlevel roundings of a sum that matters only below 745, once for the
term and once for the normalisation, doubled for the device exp.  The largest |reference - CF_x80| of the fixture is
4.05e-14 (13 levels; 1.7e-14 at 3 levels, 0 at 2): the reference's difference of two depths ~ z^2 against shares of order one."""
import os

import numpy as np
import pytest

from helpers import GOLDEN
from test_optics import DB, _bundle

pytestmark = pytest.mark.gpu

TH_TOL = 2e-13
RJUP, MJUP = 6.9911e9, 1.898e30


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLDEN, "contribfn.npz"))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "optics.npz"))


def _full(fix, nlevel, cols=None):
    """The ``full_output`` dictionary of one fixture scene (optionally its first ``cols`` columns)."""
    t = "s%d/" % nlevel
    c = slice(None) if cols is None else slice(0, cols)
    return {"wavenumber": fix[t + "wno"][c],
            "taugas": fix[t + "taugas"][:, c, None], "taucld": fix[t + "taucld"][:, c, None],
            "tauray": fix[t + "tauray"][:, c, None],
            "layer": {k: fix["%slayer/%s" % (t, k)] for k in ("pressure", "temperature", "column_density", "mmw")},
            "level": {k: fix["%slevel/%s" % (t, k)] for k in ("pressure", "temperature", "z", "dz")}}


def _check_thermal(got, ref):
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.all(got[ref == 0] == 0)
    m = np.abs(ref) >= 1e-290
    err = np.abs(got[m] - ref[m]) / np.abs(ref[m])
    print("thermal: %d values, max rel %.3e" % (err.size, err.max() if err.size else 0.0))
    assert np.all(err <= TH_TOL)


@pytest.mark.parametrize("nlevel", [13, 3, 2])
def test_thermal_matches_the_reference(fix, nlevel):
    from picaso_amd import justdoit as jdi
    full = _full(fix, nlevel)
    for tm in fix["tau_maxes"]:
        out = jdi.thermal_contribution(full, tau_max=float(tm), R=None)
        assert list(out) == ["wavenumber", "pressure", "CF"]
        assert np.array_equal(out["pressure"], full["layer"]["pressure"][:-1])
        assert np.array_equal(out["wavenumber"], full["wavenumber"])
        _check_thermal(out["CF"], fix["s%d/th_cf/%g" % (nlevel, tm)])
    if nlevel == 2:
        assert out["CF"].shape == (0, 150)
        assert jdi.thermal_contribution(full, R=int(fix["R"]))["CF"].shape[0] == 0
        return
    R = int(fix["R"])
    binned = jdi.thermal_contribution(full, tau_max=1.0, R=R)
    ref = fix["s%d/th_cf_bin" % nlevel]
    counts = fix["s%d/bin_counts" % nlevel]
    assert (counts == 0).any() and (counts == 1).any()
    assert np.array_equal(binned["wavenumber"], fix["s%d/bin_wavenumber" % nlevel])
    _check_thermal(binned["CF"], ref)
    rows = jdi.thermal_contribution(full, tau_max=1.0, R=None)["CF"]
    for r in range(rows.shape[0]):            # the binning is bit for bit
        host = jdi.mean_regrid(full["wavenumber"], rows[r], newx=binned["wavenumber"])[1]
        assert np.array_equal(binned["CF"][r], host, equal_nan=True), r


@pytest.mark.parametrize("nlevel", [91, 2])
def test_thermal_is_the_numpy_formula_on_synthetic_planes(nlevel):
    from picaso_amd import fluxes
    from picaso_amd import justdoit as jdi
    from picaso_amd import synthetic as syn
    nlayer, nwno = nlevel - 1, 150
    sc = syn.make_scene(nlayer, nwno, seed=5)
    p = sc["plevel"] / 1e6
    full = {"wavenumber": sc["wno"], "taugas": sc["taugas"], "taucld": sc["taucld"], "tauray": sc["tauray"],
            "layer": {"pressure": np.sqrt(p[1:] * p[:-1]), "temperature": 0.5 * (sc["tlevel"][1:] + sc["tlevel"][:-1])},
            "level": {"pressure": p, "temperature": sc["tlevel"]}}
    got = jdi.thermal_contribution(full, tau_max=1.0, R=None)["CF"]
    t = (sc["taugas"] + sc["taucld"]) + sc["tauray"]
    t[t > 1.0] = 1.0
    s = np.cumsum(t, axis=0)
    bb = fluxes.blackbody(full["layer"]["temperature"], 1 / sc["wno"])
    with np.errstate(all="ignore"):
        ref = bb[:-1] * np.exp(-s[:-1]) * t[:-1] / np.diff(np.log(full["layer"]["pressure"]))[:, None]
    assert got.shape == (nlayer - 1, nwno)
    _check_thermal(got, ref)


@pytest.mark.parametrize("nlevel", [13, 3, 2])
def test_transmission_matches_the_extended_precision_restatement(fix, nlevel):
    from picaso_amd import justdoit as jdi
    full = _full(fix, nlevel)
    out = jdi.transmission_contribution(full, as_reference=True)
    got, x80, ref = out["CF"], fix["s%d/tr_cf_x80" % nlevel], fix["s%d/tr_cf_ref" % nlevel]
    col_opaque, col_zero, col_nan = (int(c) for c in fix["cols"])
    assert got.shape == (nlevel - 1, 150) and np.array_equal(out["pressure"], full["layer"]["pressure"])
    assert np.array_equal(np.isnan(got), np.isnan(x80))
    assert np.isnan(got[:, col_zero]).all() and np.isfinite(got[:, col_opaque]).all()
    bound = 4 * nlevel * 745 * 2.0 ** -53
    m = x80 >= 1e-280
    err = np.abs(got[m] - x80[m]) / x80[m]
    print("transmission %d levels: max rel %.3e (bound %.3e)" % (nlevel, err.max(), bound))
    assert np.all(err <= bound)
    assert np.all(got[x80 == 0] == 0)
    ok = ~np.isnan(x80[0])
    assert np.all(np.abs(got[:, ok].sum(axis=0) - 1.0) <= nlevel * 2.0 ** -52)
    # consistency with the reference's own figure: no further from it than the restatement is, plus the bound
    assert np.all(np.abs(got[:, ok] - ref[:, ok]) <= np.abs(ref[:, ok] - x80[:, ok]) + bound * x80[:, ok])


def test_transmission_in_the_units_of_the_spectrum(fix):
    """CF[k] S = norm - F_k of two get_transit_1d calls with picaso()'s arguments, to the difference's own conditioning."""
    from picaso_amd import fluxes
    from picaso_amd import justdoit as jdi
    from picaso_amd.atmsetup import _Consts as c
    nlevel = 13
    full = _full(fix, nlevel)
    got = jdi.transmission_contribution(full)["CF"]
    dtau = (full["taugas"][:, :, 0] + full["taucld"][:, :, 0]) + full["tauray"][:, :, 0]
    lev, lay = full["level"], full["layer"]

    def depth(d):
        return fluxes.get_transit_1d(lev["z"], lev["dz"], nlevel, 150, 1.0, lay["mmw"], c.k_b, c.amu, lev["pressure"] * c.pconv,
                                     lev["temperature"], lay["column_density"], d)
    norm = depth(dtau)
    diffs = []
    for k in range(nlevel - 1):
        d = dtau.copy()
        d[k] = 0
        diffs.append(norm - depth(d))
    diffs = np.array(diffs)
    S = diffs.sum(axis=0)
    cols = [c_ for c_ in range(150) if c_ not in [int(v) for v in fix["cols"]]]
    checked = 0
    for k in (2, 6, 10):
        cond = nlevel * 2.0 ** -52 * norm[cols] / diffs[k, cols]
        use = (cond > 0) & (cond < 1e-6)
        assert use.sum() > 50, (k, use.sum())
        rel = np.abs(got[k, cols] * S[cols] - diffs[k, cols]) / diffs[k, cols]
        print("layer %d: %d columns, max rel / bound %.3f" % (k, use.sum(), (rel[use] / cond[use]).max()))
        assert np.all(rel[use] <= cond[use]), k
        checked += int(use.sum())
    assert checked > 150
    ref_units = jdi.transmission_contribution(full, as_reference=True)["CF"]
    assert np.nanmax(np.abs(ref_units - got)) > 1e-3                  # the units matter


def test_bits_do_not_depend_on_the_launch_shape(fix):
    from picaso_amd import justdoit as jdi
    whole, part = _full(fix, 13), _full(fix, 13, cols=70)
    for fn, kw in ((jdi.thermal_contribution, {"R": None}), (jdi.transmission_contribution, {"as_reference": True}),
                   (jdi.transmission_contribution, {})):
        a, b = fn(whole, **kw)["CF"], fn(part, **kw)["CF"]
        assert b.shape[1] == 70 and np.array_equal(a[:, :70], b, equal_nan=True)


def _case(gold, jdi):
    case = _bundle(gold, jdi, None, True, 2, 2)
    case.gravity(radius=RJUP, mass=MJUP)
    return case


def test_case_form_equals_dictionary_form(gold):
    from picaso_amd import justdoit as jdi
    opa = jdi.opannection(filename_db=DB, query_method="linear")
    case = _case(gold, jdi)
    before = case.spectrum(opa, calculation="thermal")
    full = case.spectrum(opa, calculation="thermal", full_output=True)["full_output"]
    for fn, kws in ((jdi.thermal_contribution, ({}, {"R": None}, {"tau_max": 50.0, "R": 30})),
                    (jdi.transmission_contribution, ({}, {"as_reference": True}, {"R": 30}))):
        for kw in kws:
            a, b = fn(case, opa, **kw), fn(full, **kw)
            for k in ("wavenumber", "pressure", "CF"):
                assert np.array_equal(a[k], b[k], equal_nan=True), (fn.__name__, kw, k)
            assert np.isfinite(a["CF"]).any()
    after = case.spectrum(opa, calculation="thermal")
    assert set(before) == set(after)
    for k, v in before.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, after[k]), k


def test_errors(gold, fix):
    from picaso_amd import justdoit as jdi
    from picaso_amd._lib import PicasoHipError
    from test_ck_optics import _case as _ck_case
    from test_ck_optics import _ck_class
    opa = jdi.opannection(filename_db=DB, query_method="linear")
    case = _case(gold, jdi)
    ck = _ck_class(np.load(os.path.join(GOLDEN, "ck.npz")))
    for fn in (jdi.thermal_contribution, jdi.transmission_contribution):
        with pytest.raises(NotImplementedError):
            fn(_ck_case(gold, jdi), ck)
        with pytest.raises(NotImplementedError):
            fn(case, opa, dimension="3d")
    full = _full(fix, 13)
    with pytest.raises(NotImplementedError):
        jdi.thermal_contribution(dict(full, taugas=np.repeat(full["taugas"], 2, axis=2)))
    no_radius = _bundle(gold, jdi, None, True, 2, 2)
    with pytest.raises(Exception, match="transmission needs the stellar radius"):
        jdi.transmission_contribution(no_radius, opa)
    # past the LDS tile: a clean error before anything is launched
    n = 140
    z = 7e9 + np.linspace(5e8, 0, n)
    tall = {"wavenumber": np.linspace(2000.0, 2100.0, 8), "taugas": np.full((n - 1, 8), 0.01),
            "taucld": np.zeros((n - 1, 8)), "tauray": np.zeros((n - 1, 8)),
            "layer": {"pressure": np.logspace(-5, 1, n - 1), "temperature": np.full(n - 1, 500.0),
                      "column_density": np.ones(n - 1), "mmw": np.full(n - 1, 2.3)},
            "level": {"pressure": np.logspace(-5, 1, n), "temperature": np.full(n, 500.0), "z": z,
                      "dz": np.full(n, z[0] - z[1])}}
    with pytest.raises(PicasoHipError, match="levels exceed the LDS tile"):
        jdi.transmission_contribution(tall)
    assert jdi.thermal_contribution(tall, R=None)["CF"].shape == (n - 2, 8)      # the context still works
