"""jdi.photon_attenuation / taumap / heatmap_taus / cloud_optics_1d on the GPU (csrc/attenuation.hip) against
tests/golden/attenuation.npz: the reference's justplotit.photon_attenuation, taumap, heatmap_taus and the np.mean lines of
all_optics_1d on synthetic ``full_output`` dictionaries (tests/golden/make_attenuation.py).

Bounds.  Levels, pressures, maps and heat maps are compared bit for bit: the kernel forms np.cumsum's sequential sums
and gathers host values; the binning is picaso_mean_regrid_plane_dev's, the logarithm numpy's own.  The band means differ
from np.mean's pairwise sums in the order of the additions alone: both sums lie within (n - 1) 2^-53 sum|x| of the exact
one, so the means differ by at most 2 (n - 1) 2^-53 mean|x|, n the window's column count."""
import os

import numpy as np
import pytest

from helpers import GOLDEN
from test_optics import DB, _bundle

pytestmark = pytest.mark.gpu

SCENES = {"s13": (13, 1), "s3": (3, 1), "s2": (2, 1), "ck13": (13, 3)}
COMP = ("gas", "cld", "ray")


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLDEN, "attenuation.npz"))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "optics.npz"))


def _full(fix, name, cols=None):
    """The ``full_output`` dictionary of one fixture scene (optionally its first ``cols`` columns)."""
    t = name + "/"
    c = slice(None) if cols is None else slice(0, cols)
    cloud = {k: fix[t + "cloud/" + k][:, c] for k in ("opd", "w0", "g0") if t + "cloud/" + k in fix.files}
    return {"wavenumber": fix[t + "wno"][c], "taugas": fix[t + "taugas"][:, c], "taucld": fix[t + "taucld"][:, c],
            "tauray": fix[t + "tauray"][:, c], "layer": {"pressure": fix[t + "layer/pressure"], "cloud": cloud},
            "level": {"pressure": fix[t + "level/pressure"]}}


def _map_full(fix):
    return {"wavenumber": fix["map/wno"], "taugas": fix["map/taugas"], "taucld": fix["map/taucld"],
            "tauray": fix["map/tauray"], "latitude": fix["map/latitude"], "longitude": fix["map/longitude"],
            "layer": {"pressure": fix["map/layer/pressure"],
                      "cloud": {k: fix["map/cloud/" + k] for k in ("opd", "w0", "g0")}},
            "level": {"pressure": fix["map/level/pressure"]}}


def _nan_col(fix):
    return int(fix["cols"][list(fix["col_names"]).index("nan")])


def _dominant(p):
    """The three np.where masks of justplotit.py:509-511 as one code."""
    g, c, r = p
    dom = np.full(g.size, -1)
    dom[(g < c) & (g < r)] = 0
    dom[(c < g) & (c < r)] = 1
    dom[(r < c) & (r < g)] = 2
    return dom


@pytest.mark.parametrize("name", list(SCENES))
def test_photon_attenuation_matches_the_reference(fix, name):
    from picaso_amd import justdoit as jdi
    full, nan_col = _full(fix, name), _nan_col(fix)
    ok = np.arange(150) != nan_col
    for at in fix["at_taus"]:
        for ig in range(SCENES[name][1]):
            out = jdi.photon_attenuation(full, at_tau=float(at), igauss=ig)
            assert list(out) == ["wavenumber", "wavelength", "pressure_gas", "pressure_cld", "pressure_ray", "level_gas",
                                 "level_cld", "level_ray", "dominant"]
            assert np.array_equal(out["wavenumber"], full["wavenumber"])
            assert np.array_equal(out["wavelength"], 1e4 / full["wavenumber"])
            ref_p, ref_l = fix["%s/pa/%g/%d/pressure" % (name, at, ig)], fix["%s/pa/%g/%d/level" % (name, at, ig)]
            for i, k in enumerate(COMP):
                assert out["level_" + k].dtype.kind == "i"
                assert np.array_equal(out["level_" + k][ok], ref_l[i, ok]), (at, ig, k)
                assert np.array_equal(out["pressure_" + k][ok], ref_p[i, ok]), (at, ig, k)
            assert np.array_equal(out["dominant"][ok], _dominant(ref_p)[ok]), (at, ig)
            # the NaN sits in the gas plane: level -1, pressure NaN, nobody dominates; cloud and Rayleigh are untouched
            assert out["level_gas"][nan_col] == -1 and np.isnan(out["pressure_gas"][nan_col])
            assert out["dominant"][nan_col] == -1
            for i, k in ((1, "cld"), (2, "ray")):
                assert out["level_" + k][nan_col] == ref_l[i, nan_col] and out["pressure_" + k][nan_col] == ref_p[i, nan_col]
    if name == "s13":
        assert set(np.unique(jdi.photon_attenuation(full, at_tau=0.5)["dominant"])) >= {0, 1}


def test_the_gauss_point_is_the_stride_of_the_gas_plane(fix):
    from picaso_amd import justdoit as jdi
    full = _full(fix, "ck13")
    a, b = (jdi.photon_attenuation(full, at_tau=1.0, igauss=ig) for ig in (0, 2))
    ok = np.arange(150) != _nan_col(fix)
    assert not np.array_equal(a["level_gas"][ok], b["level_gas"][ok])
    assert np.array_equal(a["level_ray"], b["level_ray"]) and np.array_equal(a["level_cld"], b["level_cld"])
    with pytest.raises(Exception, match="Gauss point"):
        jdi.photon_attenuation(full, igauss=3)


@pytest.mark.parametrize("cols", [64, 65, 1])
def test_the_partial_tile_is_guarded(fix, cols):
    from picaso_amd import justdoit as jdi
    for name in ("s13", "ck13"):
        ig = SCENES[name][1] - 1
        whole = jdi.photon_attenuation(_full(fix, name), at_tau=0.5, igauss=ig)
        part = jdi.photon_attenuation(_full(fix, name, cols=cols), at_tau=0.5, igauss=ig)
        for k, v in part.items():
            assert v.shape == (cols,) and np.array_equal(v, whole[k][:cols], equal_nan=True), (name, k)


@pytest.mark.parametrize("name", ["s13", "s2"])
def test_binned_pressures_are_mean_regrid_of_the_rows(fix, name):
    from picaso_amd import justdoit as jdi
    full, R = _full(fix, name), int(fix["R"])
    rows = jdi.photon_attenuation(full, at_tau=0.5)
    out = jdi.photon_attenuation(full, at_tau=0.5, R=R)
    assert list(out) == ["wavenumber", "wavelength", "pressure_gas", "pressure_cld", "pressure_ray"]
    empty = None
    for k in COMP:
        x, host = jdi.mean_regrid(full["wavenumber"], rows["pressure_" + k], R=R)
        assert np.array_equal(out["wavenumber"], x) and np.array_equal(out["wavelength"], 1e4 / x)
        assert np.array_equal(out["pressure_" + k], host, equal_nan=True), k
        empty = np.isnan(host) if k == "ray" else empty
    assert empty.any() and not empty.all()                    # empty bins are NaN


def _case(gold, jdi, cloudy):
    if cloudy:
        return _bundle(gold, jdi, None, True, 2, 2)
    case = jdi.inputs()
    case.phase_angle(0)
    case.gravity(gravity=float(gold["in/gravity"]))
    prof = {"pressure": gold["in/plevel_bar"], "temperature": gold["in/tlevel"]}
    for k in ("H2", "He", "H2O", "CH4"):
        prof[k] = gold["in/mix/" + k]
    case.atmosphere(df=prof)
    case.approx(raman="none", delta_eddington=True)
    return case


def _same(a, b, what):
    assert list(a) == list(b), what
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


@pytest.mark.parametrize("cloudy", [True, False])
def test_case_form_equals_dictionary_form(gold, cloudy):
    from picaso_amd import justdoit as jdi
    opa = jdi.opannection(filename_db=DB, query_method="linear")
    case = _case(gold, jdi, cloudy)
    before = case.spectrum(opa, calculation="thermal")
    out = case.spectrum(opa, calculation="thermal", full_output=True)
    for kw in ({}, {"at_tau": 1.0}, {"at_tau": 0.1, "R": 30}):
        a = jdi.photon_attenuation(case, opa, **kw)
        _same(a, jdi.photon_attenuation(out, **kw), kw)
        assert np.isfinite(a["pressure_gas"]).any()             # the test database leaves some columns of TAUGAS NaN
    a = jdi.photon_attenuation(case, opa, at_tau=0.1)
    if cloudy:
        assert np.all(a["level_cld"] < len(gold["in/tlevel"]) - 1)            # the cloud passes 0.1 above the bottom
    else:
        assert np.all(a["level_cld"] == len(gold["in/tlevel"]) - 1)          # a column of zeros: the bottom level
    for R in (0, 30):
        _same(jdi.heatmap_taus(case, opa, R=R), jdi.heatmap_taus(out, R=R), "heatmap R=%d" % R)
    wave = 1e4 / opa.wno
    win = (float(np.sort(wave)[2]), float(np.sort(wave)[-3]))
    _same(jdi.cloud_optics_1d(case, opa, wave_range=win), jdi.cloud_optics_1d(out, wave_range=win), "cloud_optics_1d")
    after = case.spectrum(opa, calculation="thermal")
    for k, v in before.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, after[k]), k


def test_correlated_k_case_equals_its_own_full_output(gold):
    from picaso_amd import justdoit as jdi
    from test_ck_optics import _case as _ck_case
    from test_ck_optics import _ck_class
    opa = _ck_class(np.load(os.path.join(GOLDEN, "ck.npz")))
    assert opa.ngauss == 4
    case = _ck_case(gold, jdi, True)
    case.surface_reflect(0.2)
    out = case.spectrum(opa, calculation="reflected+thermal", full_output=True)
    assert out["full_output"]["taugas"].shape[2] == 4
    levels = []
    for ig in (0, 3):
        a = jdi.photon_attenuation(case, opa, at_tau=0.5, igauss=ig)
        _same(a, jdi.photon_attenuation(out, at_tau=0.5, igauss=ig), "igauss=%d" % ig)
        levels.append(a["level_gas"])
    assert not np.array_equal(levels[0], levels[1])
    with pytest.raises(Exception, match="Gauss point"):
        jdi.photon_attenuation(case, opa, igauss=4)


def test_taumap_matches_the_reference_with_its_quirk(fix):
    from picaso_amd import justdoit as jdi
    full = _map_full(fix)
    plev = full["level"]["pressure"]
    for wl in fix["map/wavelengths"]:
        for ig in range(2):
            for at in fix["at_taus"]:
                out = jdi.taumap(full, at_tau=float(at), wavelength=float(wl), igauss=ig)
                assert list(out) == ["map_gas", "map_cld", "map_ray", "latitude", "longitude"]
                ref = fix["map/taumap/%g/%d/%g" % (wl, ig, at)]
                for i, k in enumerate(COMP):
                    assert out["map_" + k].shape == (3, 2)
                    assert np.array_equal(out["map_" + k], ref[i]), (wl, ig, at, k)
                # the quirk: a cloud that is non-zero in the first layer is put at the bottom whatever at_tau is
                assert out["map_cld"][1, 0] == plev[-1, 1, 0]
    assert np.array_equal(out["latitude"], full["latitude"]) and np.array_equal(out["longitude"], full["longitude"])
    assert jdi.taumap(full, at_tau=0.5)["map_cld"][0, 0] == plev[3, 0, 0]     # a clear top is not
    with pytest.raises(Exception, match="3-D run"):
        jdi.taumap(_full(fix, "s13"))


@pytest.mark.parametrize("name", list(SCENES))
def test_heatmap_taus_matches_the_reference(fix, name):
    from picaso_amd import justdoit as jdi
    full = _full(fix, name)
    for R in (0, int(fix["R"])):
        out = jdi.heatmap_taus({"wavenumber": full["wavenumber"], "full_output": full}, R=R)
        assert list(out) == ["wavenumber", "pressure", "taugas", "taucld", "tauray"]
        assert np.array_equal(out["wavenumber"], fix["%s/heat/R%d/wavenumber" % (name, R)])
        assert np.array_equal(out["pressure"], full["layer"]["pressure"])
        for k in ("taugas", "taucld", "tauray"):
            ref = fix["%s/heat/R%d/%s" % (name, R, k)]
            assert np.array_equal(np.isnan(out[k]), np.isnan(ref)), (R, k)
            assert np.array_equal(out[k], ref, equal_nan=True), (R, k)
    assert np.isnan(out["tauray"]).any()


def _check_means(got, fix, tag, full_cloud, lo_hi):
    lo, hi = lo_hi
    n = hi - lo
    for k in ("opd", "w0", "g0"):
        ref = fix[tag + k]
        assert got[k].shape == ref.shape
        if n == 0:
            assert np.isnan(got[k]).all() and np.isnan(ref).all()
        elif n == 1:
            assert np.array_equal(got[k], ref) and np.array_equal(got[k], full_cloud[k][:, lo])
        else:
            bound = 2 * (n - 1) * 2.0 ** -53 * np.abs(full_cloud[k][:, lo:hi]).mean(axis=1)
            err = np.abs(got[k] - ref)
            print("%s%s: n = %d, max err / bound %.3f" % (tag, k, n, np.max(err / np.where(bound > 0, bound, 1.0))))
            assert np.all(err <= bound), k


def test_cloud_optics_1d_matches_the_reference(fix):
    from picaso_amd import justdoit as jdi
    from picaso_amd.attenuation import contiguous_window
    for name in ("s13", "s2"):
        full = _full(fix, name)
        for i, win in enumerate(fix["windows"]):
            out = jdi.cloud_optics_1d(full, wave_range=tuple(win))
            assert list(out) == ["pressure", "opd", "w0", "g0"]
            assert np.array_equal(out["pressure"], full["layer"]["pressure"])
            lo_hi = contiguous_window(full["wavenumber"], win)
            assert lo_hi[1] - lo_hi[0] == int(fix["%s/optics/%d/count" % (name, i)])
            _check_means(out, fix, "%s/optics/%d/" % (name, i), full["layer"]["cloud"], lo_hi)
    full = _map_full(fix)                                     # one facet of a 3-D dictionary
    facet = {k: v[:, :, 2, 1] for k, v in full["layer"]["cloud"].items()}
    facet10 = {k: v[:, :, 1, 0] for k, v in full["layer"]["cloud"].items()}
    for i, win in enumerate(fix["map/windows"]):
        out = jdi.cloud_optics_1d(full, wave_range=tuple(win), ng=2, nt=1)
        assert np.array_equal(out["pressure"], full["layer"]["pressure"][:, 2, 1])
        _check_means(out, fix, "map/f21/optics/%d/" % i, facet, contiguous_window(full["wavenumber"], win))
    other = jdi.cloud_optics_1d(full, wave_range=tuple(fix["map/windows"][0]), ng=1, nt=0)
    lo, hi = contiguous_window(full["wavenumber"], fix["map/windows"][0])
    assert np.allclose(other["w0"], facet10["w0"][:, lo:hi].mean(axis=1), rtol=1e-14, atol=0)
    assert not np.array_equal(other["w0"], jdi.cloud_optics_1d(full, wave_range=tuple(fix["map/windows"][0]), ng=2, nt=1)["w0"])
    with pytest.raises(Exception, match="both ng and nt"):
        jdi.cloud_optics_1d(full, wave_range=(0.9, 1.1), ng=1)
