"""The inputs of tests/test_transit_levels_gpu.py are fair, checked without a GPU: at every level count that module runs,
in both calling conventions of get_transit_1d (contribfn_cases.CONVENTIONS), the double-precision oracle lies within the
derived depth bound (contribfn_cases.depth_bound) of the np.longdouble restatement, only the deliberate columns are NaN,
and no contribution share lies in (1e-400, 1e-280), where a float64 result may be a denormal, a zero or neither; the
oracle's correlated-k sum lies within that bound summed with the Gauss weights, and the saturated scenes are finite.  And the
scenes moved to contribfn_cases.py are those of the fixture tests/golden/contribfn.npz, bit for bit."""
import os

import numpy as np
import pytest

import contribfn_cases as cc
from contribfn_cases import CF_LEVELS, DEPTH_LEVELS
from helpers import GOLDEN

PLAIN = np.array([c not in (cc.COL_ZERO, cc.COL_NAN) for c in range(cc.NWNO)])


def test_extended_precision_is_extended():
    assert np.finfo(np.longdouble).nmant >= 63 and np.finfo(np.longdouble).maxexp >= 16384


@pytest.mark.parametrize("nlevel", [13, 3, 2])
def test_scene_is_the_fixtures(nlevel):
    fix = np.load(os.path.join(GOLDEN, "contribfn.npz"))
    full, t = cc.scene(nlevel), "s%d/" % nlevel

    def same(a, b):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()      # NaN payloads included
    assert same(full["wavenumber"], fix[t + "wno"])
    for k in ("taugas", "taucld", "tauray"):
        assert same(np.ascontiguousarray(full[k][:, :, 0]), fix[t + k]), k
    for grp in ("layer", "level"):
        assert sorted(full[grp]) == sorted(k.split("/")[-1] for k in fix.files if k.startswith(t + grp + "/"))
        for k, v in full[grp].items():
            assert same(v, fix["%s%s/%s" % (t, grp, k)]), (grp, k)
    assert [cc.COL_OPAQUE, cc.COL_ZERO, cc.COL_NAN] == [int(c) for c in fix["cols"]]
    # the restatement with its new keyword arguments at their defaults is the one the fixture stores (a libm's expl may
    # differ from the generator's in the last bit of the 64-bit mantissa: one ulp of float64 is allowed for it)
    cf80 = cc.restated(nlevel, "reference", True)[2].astype(np.float64)
    want = fix[t + "tr_cf_x80"]
    assert np.array_equal(np.isnan(cf80), np.isnan(want))
    m = ~np.isnan(want)
    assert np.all(np.abs(cf80[m] - want[m]) <= 2.0 ** -52 * want[m])


def test_defaults_are_the_reference_convention():
    """The keyword arguments at their defaults change no bit, in float64 and in np.longdouble."""
    full = cc.scene(9)
    for T in (np.float64, np.longdouble):
        with np.errstate(all="ignore"):
            a, b = cc.transit_terms(full, T), cc.transit_terms(full, T, **cc.CONVENTIONS["reference"])
        for x, y in zip(a, b):
            assert x.dtype == T and np.array_equal(x, y, equal_nan=True)
    with np.errstate(all="ignore"):
        assert cc.transit_terms(full, np.float64, terms=False)[1] is None
        f_lay, f_lev = (cc.transit_terms(full, np.float64, terms=False, levels=lv)[0] for lv in (False, True))
    assert not np.array_equal(f_lay, f_lev, equal_nan=True)                  # the choice of arrays matters


@pytest.mark.parametrize("convention", sorted(cc.CONVENTIONS))
@pytest.mark.parametrize("nlevel", DEPTH_LEVELS)
def test_oracle_depth_is_within_the_bound(oracle, nlevel, convention):
    kw = cc.CONVENTIONS[convention]
    full, f80 = cc.restated_depth(nlevel, convention)
    F = oracle.get_transit_1d(*cc.transit_args(full, **kw))
    nan = np.arange(cc.NWNO) == cc.COL_NAN
    assert np.array_equal(np.isnan(F), nan) and np.array_equal(np.isnan(f80), nan)
    bound = cc.depth_bound(full, f80, kw["rstar"])
    ratio = (np.abs(F[~nan] - f80[~nan]) / bound[~nan]).max()
    print("%s, %d levels: oracle - x80 at most %.3f of the bound" % (convention, nlevel, ratio))
    assert ratio <= 1.0
    # the all-zero column is the planet's disk alone, the opaque one is deeper than its neighbours
    assert F[cc.COL_ZERO] == (full["level"]["z"].min() / kw["rstar"]) ** 2
    assert nlevel < 4 or F[cc.COL_OPAQUE] > max(F[cc.COL_OPAQUE - 1], F[cc.COL_OPAQUE + 1])


@pytest.mark.parametrize("convention", sorted(cc.CONVENTIONS))
@pytest.mark.parametrize("nlevel", [13, 91])
def test_oracle_depth_with_saturated_layers(oracle, nlevel, convention):
    """DTAU = inf, 1e300, 1e6 in one layer: np.exp(-inf) = 0, the depth is finite and deeper than without."""
    kw = cc.CONVENTIONS[convention]
    full = cc.saturated_scene(nlevel)
    with np.errstate(all="ignore"):
        f80 = cc.transit_terms(full, np.longdouble, terms=False, **kw)[0]
    F, plain = oracle.get_transit_1d(*cc.transit_args(full, **kw)), oracle.get_transit_1d(*cc.transit_args(cc.scene(nlevel), **kw))
    nan = np.arange(cc.NWNO) == cc.COL_NAN
    assert np.array_equal(np.isnan(F), nan) and np.array_equal(np.isnan(f80), nan) and np.isfinite(F[~nan]).all()
    assert np.all(np.abs(F[~nan] - f80[~nan]) <= cc.depth_bound(full, f80, kw["rstar"])[~nan])
    sat = [cc.COL_INF, cc.COL_HUGE, cc.COL_1E6]
    assert len(set(c // 64 for c in sat)) == 3 and np.all(F[sat] > plain[sat])
    other = np.ones(cc.NWNO, dtype=bool)
    other[sat] = False
    assert np.array_equal(F[other], plain[other], equal_nan=True)


@pytest.mark.parametrize("nlevel", [13, 91, 129, 256])
def test_oracle_correlated_k_sum_is_within_the_weighted_bound(oracle, nlevel):
    """The Gauss-point loop of justdoit.py:388-405 in float64 -- a product and a sum per point -- against the weighted sum
    of the np.longdouble depths: the depth bound summed with the weights holds it, with nothing added for the sum."""
    kw = cc.CONVENTIONS["spectrum"]
    full, want, bound = cc.ck_restated(nlevel)
    got = np.zeros(cc.NWNO)
    for s, w in zip(cc.CK_SCALES, cc.CK_WEIGHTS):
        got = got + oracle.get_transit_1d(*cc.transit_args(cc.scaled(full, s), **kw)) * w
    nan = np.arange(cc.NWNO) == cc.COL_NAN
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(want), nan)
    ratio = (np.abs(got[~nan] - want[~nan]) / bound[~nan]).max()
    print("correlated-k, %d levels: oracle - x80 at most %.3f of the bound" % (nlevel, ratio))
    assert ratio <= 1.0


def test_spectrum_convention_is_the_contribution_functions_default():
    """transmission_contribution's default form passes these constants and the level arrays (contribution.py)."""
    from picaso_amd.atmsetup import _Consts as c
    kw = cc.CONVENTIONS["spectrum"]
    assert (kw["k_b"], kw["amu"], kw["pconv"], kw["levels"]) == (c.k_b, c.amu, c.pconv, True)
    assert cc.CONVENTIONS["reference"] == dict(rstar=1.0, k_b=1.0, amu=1.0, levels=False, pconv=1.0)


def test_scaling_by_a_power_of_two_is_exact():
    full = cc.scene(13)
    for s in (0.5, 2.0):
        assert np.array_equal(cc.dtau_of(cc.scaled(full, s)), cc.dtau_of(full) * s, equal_nan=True)
    part = cc.columns(full, 70)
    assert part["wavenumber"].size == 70 and np.array_equal(cc.dtau_of(part), cc.dtau_of(full)[:, :70], equal_nan=True)


@pytest.mark.parametrize("convention", sorted(cc.CONVENTIONS))
@pytest.mark.parametrize("nlevel", CF_LEVELS)
def test_no_share_on_the_edge_of_the_double_range(nlevel, convention):
    _, _, cf80 = cc.restated(nlevel, convention, True)
    assert cf80.shape == (nlevel - 1, cc.NWNO)
    assert np.isnan(cf80[:, ~PLAIN]).all() and not np.isnan(cf80[:, PLAIN]).any()
    assert not ((cf80 > cc.CF_EDGE_LO) & (cf80 < cc.CF_EDGE_HI)).any()
    assert np.all(cf80[:, PLAIN] >= 0) and np.all(np.abs(cf80[:, PLAIN].sum(axis=0) - 1) <= 2.0 ** -60 * nlevel)
