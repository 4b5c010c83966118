"""k_transit (csrc/transit.hip) and k_transit_cf (csrc/contribfn.hip) at every level count their tiling, their table ring
and their LDS request branch on (contribfn_cases.DEPTH_LEVELS / CF_LEVELS), against the np.longdouble restatement of
get_transit_1d (contribfn_cases.transit_terms) on contribfn_cases.scene: 150 wavenumbers (two full tiles and a partial
one) with an opaque, an all-zero and a NaN column.  tests/test_transit_levels_host.py checks the same inputs without a GPU.

Bounds, both derived and neither measured.  Depth: contribfn_cases.depth_bound, 2^-52 |F| + (1.5 nlevel + 8) 2^-53 A per
column.  The correlated-k entry: that bound summed with the Gauss weights, nothing added.  Contribution function: what
test_contribfn_gpu.test_transmission_matches_the_extended_precision_restatement asserts (contribfn_cases.cf_bound).

Largest error / bound observed on an MI355X (printed by the tests, `pytest -s`), reference / spectrum convention:

  levels   2     3     4     5     6     7     8     9     12    13    16    17    89    90    91    128   129   255   256
  depth   .263  .294  .308  .342  .306  .280  .320  .290  .265  .269  .253  .371  .175  .136  .142  .125  .124  .089  .101
          .562  .646  .657  .649  .622  .615  .620  .599  .569  .569  .535  .534  .330  .283  .292  .282  .270  .177  .186
  padded plane: the dense call's bits, so the spectrum row; correlated-k .768 (13), .420 (91), .381 (129), .269 (256),
  the oracle's Gauss-point loop gives the same four figures (test_transit_levels_host.py);
  saturated layers .269 / .569 (13), .142 / .292 (91) -- the plain scene's worst column, the saturated ones are closer

  levels         2     3       8       9       10      17      51      52      64      89      90      91      127     128
  contribution   0    .10059  .00028  .00082  .00084  .00091  .00082  .00079  .00093  .00060  .00063  .00061  .00083  .00081
                 0    .00056  .00023  .00051  .00028  .00056  .00016  .00011  .00007  .00011  .00013  .00024  .00012  .00007

The depth figures are those of the double-precision oracle against np.longdouble to three digits at every level count
(the kernel differs from the oracle by one ulp of F in a column or two of four scenes): what is left is the distance of
float64 from x87, mostly the one rounding of F itself.  The contribution function sits three orders inside its bound
everywhere but at 3 levels in the reference's convention, 1e-13 relative on a share of 3e-141 behind 320 e-foldings.

What the saturated-layer test found: before the clamp of exp's argument at 800 in k_transit, the columns with DTAU = inf
and DTAU = 1e300 came back NaN (the reference's depth is finite); the column with 1e6 was right before and after.  That
the clamp changed no bit of any other column of these scenes was recorded once, from the two builds; no test
here can repeat it.
"""
import numpy as np
import pytest

import contribfn_cases as cc
from contribfn_cases import CF_LEVELS, COL_NAN, COL_ZERO, DEPTH_LEVELS, NWNO

pytestmark = pytest.mark.gpu

PAD = 37                       # columns of NaN behind every row of a padded plane
TILE_ERROR = "levels exceed the LDS tile"
NAN_COL = np.arange(NWNO) == COL_NAN


# ---------------------------------------------------------------------------------------------- calls
def _depth(full, convention):
    from picaso_amd import fluxes
    return fluxes.get_transit_1d(*cc.transit_args(full, **cc.CONVENTIONS[convention]))


def _padded(dtau, pitch):
    plane = np.full((dtau.shape[0], pitch), np.nan)
    plane[:, :dtau.shape[1]] = dtau
    return plane


def _dev_call(name, full, convention, out_shape, pitch=None, fill=-7.0):
    """``picaso_get_transit_1d_dev`` / ``picaso_transit_cf_dev`` on a resident plane of row pitch ``pitch`` whose padding
    is NaN.  Returns ``(status, ctx, out)``; ``out`` has ``PAD`` more elements than the result, all preset to ``fill``."""
    from picaso_amd import _lib
    from picaso_amd._lib import f64, load, ptr
    from picaso_amd.device import DeviceArray
    z, dz, nlevel, nwno, rstar, mmw, k_b, amu, player, tlayer, colden, dtau = cc.transit_args(full, **cc.CONVENTIONS[convention])
    pitch = nwno if pitch is None else pitch
    ctx = _lib.context()
    d = DeviceArray.from_host(_padded(dtau, pitch), ctx)
    out = DeviceArray.from_host(np.full(int(np.prod(out_shape)) + PAD, fill), ctx)
    status = getattr(load(), name)(ctx, ptr(f64(z)), ptr(f64(dz)), nlevel, nwno, pitch, rstar, ptr(f64(mmw)), k_b, amu,
                                   ptr(f64(player)), ptr(f64(tlayer)), ptr(f64(colden)), ptr(d.addr), ptr(out.addr))
    return status, ctx, out


def _dev(name, full, convention, out_shape, pitch=None):
    from picaso_amd._lib import check
    status, ctx, out = _dev_call(name, full, convention, out_shape, pitch)
    check(status, ctx)
    host = out.to_host()
    n = int(np.prod(out_shape))
    assert np.all(host[n:] == -7.0)                      # nothing written behind the result
    return host[:n].reshape(out_shape)


# ---------------------------------------------------------------------------------------------- checks
def _check_depth(F, f80, bound, what, nan=NAN_COL):
    assert F.shape == f80.shape and np.array_equal(np.isnan(F), nan) and np.array_equal(np.isnan(f80), nan)
    assert np.isfinite(F[~nan]).all()
    ratio = float((np.abs(F[~nan] - f80[~nan]) / bound[~nan]).max())
    print("depth %s: error / bound %.3f" % (what, ratio))
    assert ratio <= 1.0, what


def _check_cf(got, cf80, nlevel, what):
    """The assertions of test_contribfn_gpu.test_transmission_matches_the_extended_precision_restatement."""
    x80 = cf80.astype(np.float64)
    assert got.shape == (nlevel - 1, NWNO)
    assert np.array_equal(np.isnan(got), np.isnan(x80))
    assert np.isnan(got[:, COL_ZERO]).all() and np.isfinite(got[:, cc.COL_OPAQUE]).all()
    bound = cc.cf_bound(nlevel)
    m = x80 >= 1e-280
    err = np.abs(got[m] - x80[m]) / x80[m]
    print("contribution %s: error / bound %.5f (max rel %.3e)" % (what, err.max() / bound, err.max()))
    assert np.all(err <= bound)
    assert np.all(got[x80 == 0] == 0)
    ok = ~np.isnan(x80[0])
    assert ok.sum() == NWNO - 2
    assert np.all(np.abs(got[:, ok].sum(axis=0) - 1.0) <= nlevel * 2.0 ** -52)


# ---------------------------------------------------------------------------------------------- the depth
@pytest.mark.parametrize("nlevel", DEPTH_LEVELS)
def test_depth_at_every_layout(nlevel):
    for convention, kw in sorted(cc.CONVENTIONS.items()):
        full, f80 = cc.restated_depth(nlevel, convention)
        F = _depth(full, convention)
        _check_depth(F, f80, cc.depth_bound(full, f80, kw["rstar"]), "%s, %d levels" % (convention, nlevel))
        assert F[COL_ZERO] == (full["level"]["z"].min() / kw["rstar"]) ** 2          # the disk alone: 1 - exp(-0) = 0


@pytest.mark.parametrize("nlevel", [13, 91, 129, 256])
def test_depth_on_a_padded_plane(nlevel):
    """A row pitch above nwno, the padding NaN: no NaN leaks in and the bits are those of the dense call."""
    full, f80 = cc.restated_depth(nlevel, "spectrum")
    dense = _depth(full, "spectrum")
    padded = _dev("picaso_get_transit_1d_dev", full, "spectrum", (NWNO,), pitch=NWNO + PAD)
    assert np.array_equal(np.isnan(padded), NAN_COL)
    assert np.array_equal(padded, dense, equal_nan=True)
    _check_depth(padded, f80, cc.depth_bound(full, f80, cc.CONVENTIONS["spectrum"]["rstar"]), "padded, %d levels" % nlevel)


@pytest.mark.parametrize("nlevel", [13, 91, 129, 256])
def test_depth_correlated_k(nlevel):
    """picaso_get_transit_1d_ck_dev with three Gauss points whose optical depths are 1/2, 1 and 2 times the scene's."""
    from picaso_amd import _lib, resident
    from picaso_amd.device import DeviceArray
    full, want, bound = cc.ck_restated(nlevel)
    z, dz, n, nwno, rstar, mmw, k_b, amu, player, tlayer, colden, dtau = cc.transit_args(full, **cc.CONVENTIONS["spectrum"])
    ctx = _lib.context()
    plane = np.stack([dtau * s for s in cc.CK_SCALES], axis=2).reshape(n - 1, nwno * 3)      # the Gauss index fastest
    out = DeviceArray((nwno,), ctx)
    resident.transit_1d_ck(ctx, z, dz, n, nwno, 3, rstar, mmw, k_b, amu, player, tlayer, colden,
                           DeviceArray.from_host(plane, ctx), cc.CK_WEIGHTS, out)
    _check_depth(out.to_host(), want, bound, "correlated-k, %d levels" % nlevel)


def test_depth_refuses_257_levels():
    from picaso_amd._lib import PicasoHipError, check
    full = cc.scene(257)
    status, ctx, out = _dev_call("picaso_get_transit_1d_dev", full, "spectrum", (NWNO,), fill=-3.0)
    assert status != 0
    with pytest.raises(PicasoHipError, match=TILE_ERROR):
        check(status, ctx)
    assert np.all(out.to_host() == -3.0)                                  # nothing was launched
    with pytest.raises(PicasoHipError, match=TILE_ERROR):
        _depth(full, "spectrum")
    small, f80 = cc.restated_depth(13, "spectrum")                    # the context still works
    _check_depth(_depth(small, "spectrum"), f80, cc.depth_bound(small, f80, cc.CONVENTIONS["spectrum"]["rstar"]),
                 "13 levels after the refusal")


@pytest.mark.parametrize("convention", sorted(cc.CONVENTIONS))
@pytest.mark.parametrize("nlevel", [13, 91])
def test_depth_with_saturated_layers(nlevel, convention):
    """A layer of DTAU = inf, 1e300 or 1e6: exp(-TAUALL) of every chord through it is 0, as np.exp(-inf) is, and the depth
    is finite; the NaN column stays NaN; no other column changes a bit."""
    kw = cc.CONVENTIONS[convention]
    full = cc.saturated_scene(nlevel)
    with np.errstate(all="ignore"):
        f80 = cc.transit_terms(full, np.longdouble, terms=False, **kw)[0]
    assert np.array_equal(np.isnan(f80), NAN_COL)
    F = _depth(full, convention)
    print("saturated %s, %d levels: inf %r, 1e300 %r, 1e6 %r" % (convention, nlevel, F[cc.COL_INF], F[cc.COL_HUGE], F[cc.COL_1E6]))
    _check_depth(F, f80, cc.depth_bound(full, f80, kw["rstar"]), "saturated %s, %d levels" % (convention, nlevel))
    plain = _depth(cc.scene(nlevel), convention)
    other = np.ones(NWNO, dtype=bool)
    other[[cc.COL_INF, cc.COL_HUGE, cc.COL_1E6]] = False
    assert np.array_equal(F[other], plain[other], equal_nan=True)
    assert np.all(F[~other] > plain[~other])


# ---------------------------------------------------------------------------------------------- the contribution function
def _cf(full, **kw):
    from picaso_amd import justdoit as jdi
    out = jdi.transmission_contribution(full, **kw)
    assert np.array_equal(out["pressure"], full["layer"]["pressure"])
    return out["CF"]


@pytest.mark.parametrize("nlevel", CF_LEVELS)
def test_contribution_at_every_layout(nlevel):
    for convention, kw in (("reference", {"as_reference": True}), ("spectrum", {})):
        full, _, cf80 = cc.restated(nlevel, convention, True)
        _check_cf(_cf(full, **kw), cf80, nlevel, "%s, %d levels" % (convention, nlevel))


@pytest.mark.parametrize("nlevel", [52, 91])
def test_contribution_on_a_padded_plane(nlevel):
    full, _, cf80 = cc.restated(nlevel, "reference", True)
    dense = _cf(full, as_reference=True)
    padded = _dev("picaso_transit_cf_dev", full, "reference", (nlevel - 1, NWNO), pitch=NWNO + PAD)
    assert np.array_equal(padded, dense, equal_nan=True)
    _check_cf(padded, cf80, nlevel, "padded, %d levels" % nlevel)


def test_contribution_refuses_129_levels():
    from picaso_amd._lib import PicasoHipError
    with pytest.raises(PicasoHipError, match=TILE_ERROR):
        _cf(cc.scene(129))
    full, _, cf80 = cc.restated(13, "reference", True)                    # the context still works
    _check_cf(_cf(full, as_reference=True), cf80, 13, "13 levels after the refusal")


# ---------------------------------------------------------------------------------------------- launch independence
def test_bits_do_not_depend_on_the_launch_shape():
    """The first 70 columns alone (a full tile and a partial one) are those columns of the whole, bit for bit."""
    full = cc.restated_depth(129, "spectrum")[0]
    whole, part = _depth(full, "spectrum"), _depth(cc.columns(full, 70), "spectrum")
    assert part.shape == (70,) and np.array_equal(whole[:70], part, equal_nan=True)
    full = cc.restated(91, "reference", True)[0]
    for kw in ({"as_reference": True}, {}):
        whole, part = _cf(full, **kw), _cf(cc.columns(full, 70), **kw)
        assert part.shape == (90, 70) and np.array_equal(whole[:, :70], part, equal_nan=True)
