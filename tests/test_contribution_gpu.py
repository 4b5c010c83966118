"""justdoit.get_contribution / compute_opacity(return_mode=True) on the GPU (reference justdoit.py:1090-1294,
optics.py:123-319): per-species planes from k_opacity_gas<3>, cumulative sums and tau-pressures from
k_contribution_columns, against tests/golden/contribution.npz (the reference's own compute_opacity(return_mode=True) +
its column pass, tests/golden/make_contribution.py) and against numpy on the returned arrays at 1e5 x 90."""
import os

import numpy as np
import pytest

from helpers import GOLDEN
from test_ck_optics import _case as _ck_case
from test_ck_optics import _ck_class
from test_optics import DB, NAMES, _bundle, _close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def contrib():
    return np.load(os.path.join(GOLDEN, "contribution.npz"))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "optics.npz"))


@pytest.fixture(scope="module")
def ck():
    return np.load(os.path.join(GOLDEN, "ck.npz"))


def _bracket(cum, x):
    """numpy.interp's bracket per column: the number of levels with cum <= x, minus one"""
    return (np.asarray(cum) <= x).sum(axis=0) - 1


def _check_against_fixture(contrib, tag, out, at_tau):
    keys = [str(k) for k in contrib[tag + "/keys"]]
    assert list(out["taus_per_layer"]) == keys
    assert list(out["cumsum_taus"]) == keys and list(out["tau_p_surface"]) == keys
    for k in keys:
        cum_ref = contrib["%s/cum/%s" % (tag, k)]
        assert _close(out["taus_per_layer"][k], contrib["%s/taus/%s" % (tag, k)], 1e-10), (tag, k)
        assert _close(out["cumsum_taus"][k], cum_ref, 1e-10), (tag, k)
        p_ref = contrib["%s/p_at/%g/%s" % (tag, at_tau, k)]
        assert _close(out["tau_p_surface"][k], p_ref, 1e-9), (tag, at_tau, k)
        assert np.array_equal(_bracket(out["cumsum_taus"][k], at_tau), _bracket(cum_ref, at_tau)), (tag, at_tau, k)


@pytest.mark.parametrize("qm", ["nearest", "linear"])
def test_contribution_matches_the_reference_monochromatic(contrib, gold, qm):
    from picaso_amd import justdoit as jdi
    opa = jdi.opannection(filename_db=DB, query_method=qm)
    case = _bundle(gold, jdi, None, True, 2, 2)
    for at_tau in contrib["at_taus"]:
        out = jdi.get_contribution(case, opa, at_tau=float(at_tau))
        _check_against_fixture(contrib, qm, out, float(at_tau))
    # at_tau = 0: the cloud's cumulative sum is 0 down to the deck -- the last tied level is the bracket
    out = jdi.get_contribution(case, opa, at_tau=0)
    top = int(np.argmax(gold["in/cld_opd"][:, 0] > 0))
    assert top > 0 and np.all(_bracket(out["cumsum_taus"]["cloud"], 0.0) == top)


def test_contribution_matches_the_reference_correlated_k(contrib, ck, gold):
    from picaso_amd import justdoit as jdi
    opa = _ck_class(ck)
    case = _ck_case(gold, jdi)
    for at_tau in contrib["at_taus"]:
        out = jdi.get_contribution(case, opa, at_tau=float(at_tau))
        _check_against_fixture(contrib, "ck", out, float(at_tau))
    # k-tables mixed on the fly: no per-molecule term either; continuum, Rayleigh and cloud as for the premixed table
    fly = jdi.get_contribution(case, _ck_class(ck, fly=True), at_tau=1.0)
    out = jdi.get_contribution(case, opa, at_tau=1.0)
    for part in ("taus_per_layer", "cumsum_taus", "tau_p_surface"):
        assert list(fly[part]) == list(out[part])
        for k in out[part]:
            assert np.array_equal(fly[part][k], out[part][k]), (part, k)


def test_contribution_full_size_is_numpy_on_its_own_planes():
    """1e5 wavelengths x 90 layers, 6 species (2 CIA pairs, 2 molecules, rayleigh, cloud slab)."""
    from picaso_amd import justdoit as jdi
    from picaso_amd import optics as px
    from picaso_amd import synthetic as syn
    from picaso_amd.spectrum import _setup_atmosphere
    nwno, nlayer = 100000, 90
    opa = px.RetrieveOpacities(query_method="linear", **syn.opacity_tables(nwno))
    case = _full_case(jdi, nlayer, nwno, cloud=True)
    out = jdi.get_contribution(case, opa, at_tau=1.0)
    keys = list(out["taus_per_layer"])
    assert keys == ["H2H2", "H2He", "H2O", "CH4", "rayleigh", "cloud"]
    atm = _setup_atmosphere(case.inputs, opa, opa.wno)
    plev = np.asarray(atm.level["pressure"], dtype=float) / atm.c.pconv
    total = 0.0
    for k in keys:
        t, c, p = out["taus_per_layer"][k], out["cumsum_taus"][k], out["tau_p_surface"][k]
        assert t.shape == (nlayer, nwno) and c.shape == (nlayer + 1, nwno) and p.shape == (nwno,)
        assert np.all(c[0] == 0) and np.array_equal(c[1:], np.cumsum(t, axis=0)), k
        want = np.array([np.interp(1.0, c[:, w], plev) for w in range(nwno)])
        assert np.array_equal(p, want), k
        total = total + t
    assert np.any(out["taus_per_layer"]["cloud"] > 0)
    opa.get_opacities(atm)
    dtau_og = px.compute_opacity(atm, opa, delta_eddington=False, raman=2, test_mode=None)[NAMES.index("dtau_og")]
    assert _close(total, dtau_og[:, :, 0], 1e-13)


def _full_case(jdi, nlayer, nwno, cloud):
    from picaso_amd import synthetic as syn
    nlevel = nlayer + 1
    plev = np.logspace(-6, 2, nlevel)
    case = jdi.inputs()
    case.phase_angle(0)
    case.gravity(gravity=2500.0)
    case.atmosphere(df={"pressure": plev, "temperature": 150.0 + 1200.0 * ((np.log10(plev) + 6) / 8) ** 2,
                        "H2": np.full(nlevel, 0.84), "He": np.full(nlevel, 0.155), "H2O": np.full(nlevel, 1e-3),
                        "CH4": np.full(nlevel, 5e-4)})
    if cloud:
        case.clouds(df=syn.cloud_slab(nlayer, nwno))
    case.approx(raman="none")
    return case


def test_contribution_edges(gold):
    from picaso_amd import justdoit as jdi
    from picaso_amd import optics as px
    from picaso_amd.spectrum import _setup_atmosphere
    opa = jdi.opannection(filename_db=DB, query_method="linear")
    plev_bottom = float(gold["in/plevel_bar"][-1])
    # cloud-free (no clouds() call): an all-zero "cloud" entry, as in the reference; the other species as with clouds
    clear = jdi.inputs()
    clear.phase_angle(0)
    clear.gravity(gravity=float(gold["in/gravity"]))
    clear.atmosphere(df=dict({"pressure": gold["in/plevel_bar"], "temperature": gold["in/tlevel"]},
                             **{k: gold["in/mix/" + k] for k in ("H2", "He", "H2O", "CH4")}))
    clear.approx(raman="none")
    out = jdi.get_contribution(clear, opa)
    assert list(out["taus_per_layer"])[-1] == "cloud"
    assert not np.any(out["taus_per_layer"]["cloud"]) and not np.any(out["cumsum_taus"]["cloud"])
    assert np.all(out["tau_p_surface"]["cloud"] == out["tau_p_surface"]["cloud"][0])     # never reaches 1: the bottom
    case = _bundle(gold, jdi, None, True, 2, 2)
    cloudy = jdi.get_contribution(case, opa)
    assert list(cloudy["taus_per_layer"]) == list(out["taus_per_layer"])
    for k in list(out["taus_per_layer"])[:-1]:
        assert np.array_equal(out["taus_per_layer"][k], cloudy["taus_per_layer"][k]), k
    # above every column's total: the bottom pressure; NaN: NaN
    high = jdi.get_contribution(case, opa, at_tau=1e300)
    nan = jdi.get_contribution(case, opa, at_tau=float("nan"))
    for k, p in high["tau_p_surface"].items():
        assert np.all(p == p[0]) and abs(p[0] - plev_bottom) <= 1e-12 * plev_bottom, k
        assert np.all(np.isnan(nan["tau_p_surface"][k])), k
    with pytest.raises(NotImplementedError):
        jdi.get_contribution(case, opa, dimension="3d")
    # compute_opacity(return_mode=True) is the same species planes, bit for bit
    out = jdi.get_contribution(case, opa, at_tau=1)
    atm = _setup_atmosphere(case.inputs, opa, opa.wno)
    opa.get_opacities(atm)
    modes = px.compute_opacity(atm, opa, return_mode=True)
    assert list(modes) == list(out["taus_per_layer"])
    for k, v in modes.items():
        assert np.array_equal(v, out["taus_per_layer"][k]), k


def test_contribution_leaves_spectra_alone(gold):
    from picaso_amd import justdoit as jdi
    opa = jdi.opannection(filename_db=DB, query_method="linear")
    case = _bundle(gold, jdi, None, True, 2, 2)
    case.surface_reflect(0.2)
    before = case.spectrum(opa, calculation="reflected+thermal")
    jdi.get_contribution(case, opa)
    after = case.spectrum(opa, calculation="reflected+thermal")
    assert set(before) == set(after)
    for k, v in before.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, after[k]), k
