"""The synthetic ``full_output`` scenes of tests/golden/contribfn.npz and the numpy restatement of get_transit_1d, shared
by the fixture's generator (tests/golden/make_contribfn.py) and the tests (test_transit_levels_host.py,
test_transit_levels_gpu.py).  Plain numpy: nothing here reads the reference.

  scene(nlevel)       150 wavenumbers (two full 64-lane tiles and a partial one); a T(p) that is not isothermal, a cloud
                      slab, one opaque layer (dtau 1e4) in column 17, column 70 all zero, one NaN in column 131
  transit_terms       get_transit_1d and the non-negative terms of its contribution function in any numpy float type,
                      for the reference's contribution-function arguments (the defaults) or the spectrum's
  depth_bound         the derived bound of a float64 transit depth against the np.longdouble restatement
"""
import functools

import numpy as np

NWNO = 150
COL_OPAQUE, COL_ZERO, COL_NAN = 17, 70, 131          # one in each 64-lane tile

# The level counts at which the transmission kernels change their work layout (csrc/transit.hip, csrc/contribfn.hip).
# k_transit: four waves take the chords i = wave, wave + 4, ..., two at a time in groups of 8 levels with a one-at-a-time
# tail (2 .. 17: fewer chords than waves, every shape of the paired group and of the tail); its chord table of
# (n^2 + 3 n - 2) 8 bytes leaves the 64 KB table ring between 89 and 90 levels; its tile passes 64 KB of LDS, which a
# launch has to ask for, between 128 and 129; 256 is the cap of both the tile and the per-lane term array, 257 is refused.
DEPTH_LEVELS = (2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 17, 89, 90, 91, 128, 129, 255, 256)
# k_transit_cf: eight waves, three planes of 1 280 bytes per level: past 64 KB of LDS between 51 and 52 levels, at the cap
# of 160 KB with 128, refused from 129; the table ring changes at 89 / 90 as above.
CF_LEVELS = (2, 3, 8, 9, 10, 17, 51, 52, 64, 89, 90, 91, 127, 128)

# the two ways get_transit_1d is called: by the reference's transmission_contribution (justplotit.py:1728-1738: layer
# pressure in bar, layer temperature, constants 1) and by the spectrum (justdoit.py:390-394: level pressure in dyn/cm^2,
# level temperature, cgs constants, the star's radius)
CONVENTIONS = {
    "reference": dict(rstar=1.0, k_b=1.0, amu=1.0, levels=False, pconv=1.0),
    "spectrum": dict(rstar=6.96e10, k_b=1.380649e-16, amu=1.66053906660e-24, levels=True, pconv=1e6),
}


def scene(nlevel):
    """A ``full_output`` dictionary with the reference's keys."""
    nlayer = nlevel - 1
    rng = np.random.default_rng(100 + nlevel)
    wno = np.concatenate((np.linspace(2000.0, 2400.0, 99), [2700.0], np.linspace(3000.0, 3300.0, 50)))
    assert wno.size == NWNO
    plev = np.logspace(-5, 1.5, nlevel)                                    # bar
    x = (np.log10(plev) + 5) / 6.5
    tlev = 220.0 + 1100.0 * x ** 1.5 - 60.0 * np.sin(3 * x)               # not isothermal
    play, tlay = np.sqrt(plev[1:] * plev[:-1]), 0.5 * (tlev[1:] + tlev[:-1])
    mmw = np.full(nlayer, 2.3) + 0.02 * np.arange(nlayer)
    k_b, amu, g, radius = 1.380649e-16, 1.66053906660e-24, 2500.0, 7.0e9
    scale_h = k_b * tlay / (mmw * amu * g)
    dz_lay = scale_h * np.log(plev[1:] / plev[:-1])
    z = radius + np.concatenate((np.cumsum(dz_lay[::-1])[::-1], [0.0]))    # decreasing, the bottom at `radius`
    dz = np.concatenate(([dz_lay[0]], dz_lay))
    # the reference's call makes every slant depth 1e-6 k_b / amu = 83 times the physical one (bar, constants 1), some
    # 5e3 times the vertical depth on this planet: the column density is scaled up so that slant depths stay of order one
    colden = 5.0e3 * (plev[1:] - plev[:-1]) * 1e6 / g
    lam = (wno - wno[0]) / (wno[-1] - wno[0])
    depth = np.diff(plev)[:, None] / plev[-1]
    taugas = 30.0 * depth ** 0.8 * 10.0 ** (1.5 * np.sin(9 * lam)[None, :] - 1.0) * rng.uniform(0.7, 1.3, (nlayer, NWNO))
    tauray = 2.0 * depth * (wno[None, :] / 3300.0) ** 4
    taucld = np.zeros((nlayer, NWNO))
    slab = slice(nlayer // 2, nlayer // 2 + max(1, nlayer // 4))
    taucld[slab] = 0.4 * (1.0 + 0.3 * lam)[None, :]
    k_opaque = nlayer // 3
    taugas[k_opaque, COL_OPAQUE] = 1e4
    taugas[:, COL_ZERO] = tauray[:, COL_ZERO] = taucld[:, COL_ZERO] = 0.0
    taugas[min(1, nlayer - 1), COL_NAN] = np.nan
    shape3 = (nlayer, NWNO, 1)
    return {"wavenumber": wno, "taugas": taugas.reshape(shape3), "taucld": taucld.reshape(shape3),
            "tauray": tauray.reshape(shape3),
            "layer": {"pressure": play, "temperature": tlay, "column_density": colden, "mmw": mmw},
            "level": {"pressure": plev, "temperature": tlev, "z": z, "dz": dz}}


COL_INF, COL_HUGE, COL_1E6 = 5, 69, 140               # saturated_scene's columns, one in each tile


def saturated_scene(nlevel):
    """``scene(nlevel)`` with one mid-atmosphere layer of taugas set to inf, 1e300 and 1e6 in three columns: every chord
    through that layer is opaque, exp(-TAUALL) is exactly 0 there and the depth stays finite."""
    full = scene(nlevel)
    gas = full["taugas"].copy()
    layer = (nlevel - 1) // 2
    gas[layer, COL_INF, 0], gas[layer, COL_HUGE, 0], gas[layer, COL_1E6, 0] = np.inf, 1e300, 1e6
    return dict(full, taugas=gas)


def columns(full, ncol):
    """The first ``ncol`` columns of a scene."""
    out = dict(full, wavenumber=full["wavenumber"][:ncol])
    for k in ("taugas", "taucld", "tauray"):
        out[k] = np.ascontiguousarray(full[k][:, :ncol])
    return out


def scaled(full, s):
    """The scene with every optical depth times ``s``, a power of two: DTAU scales exactly."""
    return dict(full, **{k: full[k] * s for k in ("taugas", "taucld", "tauray")})


def dtau_of(full):
    """DTAU as the reference adds its three planes (justplotit.py:1725-1727), float64 (nlayer, nwno)."""
    return (full["taugas"][:, :, 0] + full["taucld"][:, :, 0]) + full["tauray"][:, :, 0]


def pt_of(full, levels=False, pconv=1.0):
    """``(player, tlayer)`` of a get_transit_1d call in float64: the layer arrays, or the level arrays (``levels``) with
    the pressure times ``pconv`` -- the product rounded in float64, as the caller hands it over."""
    grp = full["level" if levels else "layer"]
    p = np.asarray(grp["pressure"], dtype=np.float64)
    return (p if pconv == 1.0 else p * pconv), np.asarray(grp["temperature"], dtype=np.float64)


def transit_args(full, rstar=1.0, k_b=1.0, amu=1.0, levels=False, pconv=1.0):
    """The positional arguments of get_transit_1d (reference fluxes.py:2582-2583) for one scene."""
    player, tlayer = pt_of(full, levels, pconv)
    dtau = dtau_of(full)
    return (full["level"]["z"], full["level"]["dz"], dtau.shape[0] + 1, dtau.shape[1], rstar, full["layer"]["mmw"], k_b, amu,
            player, tlayer, full["layer"]["column_density"], dtau)


def transit_terms(full, dtype, rstar=1, k_b=1, amu=1, levels=False, pconv=1.0, terms=True):
    """get_transit_1d (reference fluxes.py:2581-2663) restated in ``dtype``: ``(F, D)`` -- the transit depth and
    ``D[k] = sum_{i>k} z_i dz_i exp(-(TAUALL_i - c_ik)) (1 - exp(-c_ik))``, so that ``norm - F_k = 2 D[k] / rstar^2``.
    The defaults are the reference's contribution-function arguments (justplotit.py:1728-1738: layer pressure and
    temperature, constants 1); ``levels`` takes ``player`` / ``tlayer`` from the level arrays (pressure times ``pconv``), as
    the spectrum does.  ``terms=False`` leaves ``D`` out (None)."""
    T = dtype
    z, dz = full["level"]["z"].astype(T), full["level"]["dz"].astype(T)
    player, tlayer = (a.astype(T) for a in pt_of(full, levels, pconv))
    colden, mmw = full["layer"]["column_density"].astype(T), full["layer"]["mmw"].astype(T)
    dtau = dtau_of(full).astype(T)
    n = z.size
    dl = np.zeros((n, n), dtype=T)
    seg = T(0)
    for i in range(n):
        for j in range(i):
            ref, inner, outer = z[i], z[i - j], z[i - j - 1]
            if inner != ref and outer != ref:
                seg = np.sqrt(outer ** 2 - ref ** 2) - np.sqrt(inner ** 2 - ref ** 2)
            elif inner == ref:
                seg = np.sqrt(outer ** 2 - ref ** 2)
            dl[i, j] = seg * player[i - j - 1] / tlayer[i - j - 1] / T(k_b)
    tau = dtau / colden[:, None] * (mmw * T(amu))[:, None]
    tauall = np.zeros((n, dtau.shape[1]), dtype=T)
    for i in range(n):
        for j in range(i):
            tauall[i] = tauall[i] + 2 * tau[i - j - 1] * dl[i, j]
    F = (z.min() / T(rstar)) ** 2 + T(2) / (T(rstar) * T(rstar)) * ((T(1) - np.exp(-tauall)) * (z * dz)[:, None]).sum(axis=0)
    if not terms:
        return F, None
    D = np.zeros((n - 1, dtau.shape[1]), dtype=T)
    for k in range(n - 1):
        for i in range(k + 1, n):
            c = 2 * tau[k] * dl[i, i - k - 1]
            D[k] = D[k] + (z[i] * dz[i]) * np.exp(-(tauall[i] - c)) * -np.expm1(-c)
    return F, D


def depth_bound(full, f80, rstar=1.0):
    """Per column, the most a float64 evaluation of get_transit_1d may differ from the np.longdouble restatement ``f80``:

        2^-52 |F_x80| + (1.5 nlevel + 8) 2^-53 A,      A = (2 / rstar^2) sum_i |z_i dz_i|.

    A chord sum of at most nlevel non-negative terms carries at most (nlevel + 3) 2^-53 relative error, fused or not; that
    moves exp(-t) by at most 0.37 (nlevel + 3) 2^-53 (t e^-t <= 1/e); the exponential adds 2 ulp of a value <= 1, the
    subtraction and the product two roundings; the level-order sum at most (nlevel - 1) 2^-53 A; the last multiply-add
    one ulp of F."""
    L = np.longdouble
    z, dz = full["level"]["z"].astype(L), full["level"]["dz"].astype(L)
    n = z.size
    A = L(2) / (L(rstar) * L(rstar)) * np.abs(z * dz).sum()
    return L(2.0) ** -52 * np.abs(f80) + (L(1.5) * n + 8) * L(2.0) ** -53 * A


CF_EDGE_LO, CF_EDGE_HI = np.longdouble("1e-400"), 1e-280


def cf_bound(nlevel):
    """Relative, where the share is at least 1e-280: the argument of exp carries up to nlevel roundings of a sum that
    matters only below 745, once for the term and once for the normalisation, doubled for the device exp."""
    return 4 * nlevel * 745 * 2.0 ** -53


@functools.lru_cache(maxsize=None)
def restated(nlevel, convention, terms):
    """``(full, F_x80, CF_x80)`` of ``scene(nlevel)`` under one of ``CONVENTIONS``, np.longdouble, computed once per
    session and never written to; ``CF_x80`` (the shares ``D / sum_k D``) is None without ``terms``."""
    full = scene(nlevel)
    with np.errstate(all="ignore"):
        f80, d80 = transit_terms(full, np.longdouble, terms=terms, **CONVENTIONS[convention])
        cf80 = d80 / d80.sum(axis=0) if terms else None
    for a in (f80, cf80):
        if a is not None:
            a.setflags(write=False)
    return full, f80, cf80


def restated_depth(nlevel, convention):
    """``(full, F_x80)`` for a test of the depth alone.  At a level count the contribution tests run as well this is their
    cache entry (the depth is the same with or without the terms), so the scene is restated once per session, not twice."""
    return restated(nlevel, convention, nlevel in CF_LEVELS)[:2]


CK_SCALES, CK_WEIGHTS = (0.5, 1.0, 2.0), np.array([0.2, 0.5, 0.3])


@functools.lru_cache(maxsize=None)
def ck_restated(nlevel):
    """The correlated-k case: three Gauss points whose optical depths are ``CK_SCALES`` times the scene's, spectrum
    convention.  ``(full, want, bound)``: the scene, the ``CK_WEIGHTS``-weighted sum of the three np.longdouble depths
    and ``depth_bound`` summed with the same weights."""
    L = np.longdouble
    kw = CONVENTIONS["spectrum"]
    full, f80_1 = restated_depth(nlevel, "spectrum")
    want, bound = L(0), L(0)
    for s, w in zip(CK_SCALES, CK_WEIGHTS):
        fg = scaled(full, s)
        with np.errstate(all="ignore"):
            f80 = f80_1 if s == 1.0 else transit_terms(fg, L, terms=False, **kw)[0]
        want = want + L(w) * f80
        bound = bound + L(w) * depth_bound(fg, f80, kw["rstar"])
    return full, want, bound
