"""Contribution functions on the device: ``jdi.thermal_contribution`` and ``jdi.transmission_contribution``.

"Which pressures does this emission feature come from?" and "which layers set this transit depth?" -- the reference's
``justplotit.thermal_contribution`` (justplotit.py:1584-1643) and ``justplotit.transmission_contribution`` (:1697-1779)
without their figures.  Both read the three optical-depth planes of the opacity stage (``taugas``, ``taucld``, ``tauray``):
from an ``inputs`` object the planes are formed on the device and stay there, from a ``full_output`` dictionary (the
reference's calling form) they are uploaded; the same kernels (csrc/contribfn.hip) serve both and only ``CF`` -- binned
when ``R`` is given -- comes back.
"""

import numpy as np

from . import _lib, optics, regrid, resident
from .atmsetup import _Consts
from .device import DeviceArray

NEEDS_RADIUS = "transmission needs the stellar radius (star()) and the planet radius and mass (gravity())"


def cf_grid(opacityclass_or_wno, R):
    """The grid the reference bins a contribution function to: ``wavenumber = mean_regrid(wno, wno, R=R)[0]`` (the centres
    of the constant-``R`` bins) and then ``mean_regrid(wno, row, newx=wavenumber)`` for every row -- bins whose edges lie
    half way between those centres.  Returns ``(wavenumber, plan)``, ``plan`` the ``RegridPlan`` of the second call."""
    wavenumber = regrid.regrid_plan(opacityclass_or_wno, R=R).centres
    return wavenumber, regrid.regrid_plan(opacityclass_or_wno, newx=wavenumber)


def _binned(ctx, cf, wno, R, grid_of, grid=cf_grid):
    """``cf``: a ``(nrows, nwno)`` DeviceArray -> ``(wavenumber, host array)``, binned on the device when ``R`` is given.
    ``grid(grid_of, R)`` -> ``(wavenumber, plan)``: ``cf_grid`` for the contribution functions, ``attenuation.r_grid`` for
    the functions whose reference bins with ``mean_regrid(..., R=R)`` itself."""
    nrows, nwno = cf.shape
    if R is None:
        return wno, cf.to_host() if nrows else np.zeros((0, nwno))
    wavenumber, plan = grid(grid_of, R)
    if not nrows:
        return wavenumber, np.zeros((0, plan.nbins))
    out = DeviceArray((nrows, plan.nbins), ctx)
    _lib.check(_lib.load().picaso_mean_regrid_plane_dev(
        ctx, nrows, nwno, nwno, plan.nbins, plan.device_start(ctx).addr,
        _lib.ptr(cf.addr), _lib.ptr(out.addr)), ctx)
    return wavenumber, out.to_host()


NO_CK = ("contribution functions of correlated-k tables (ngauss > 1) are not defined: the reference takes one Gauss "
         "point of the planes")


def _plane(x, nlayer, nwno, ctx, igauss=None):
    """One plane of a ``full_output`` dictionary -- ``(nlayer, nwno, ngauss)`` as the reference stores it -- in HBM.
    ``igauss`` None: monochromatic planes only (``ngauss`` 1); else the Gauss point ``[:, :, igauss]``, cut out on the host."""
    a = np.asarray(x, dtype=float)
    if a.ndim == 3:
        if igauss is None:
            if a.shape[2] != 1:
                raise NotImplementedError(NO_CK)
            igauss = 0
        if not 0 <= igauss < a.shape[2]:
            raise Exception("igauss=%d, but the planes hold %d Gauss point(s)" % (igauss, a.shape[2]))
        a = a[:, :, igauss]
    if a.shape != (nlayer, nwno):
        raise Exception("contribution: a plane of shape %s, expected %s" % (a.shape, (nlayer, nwno)))
    return DeviceArray.from_host(a, ctx)


def _from_dictionary(x, igauss=None):
    """``(profile, planes, wno, grid_of, ctx)`` of a ``full_output`` dictionary (or of the dictionary ``spectrum(...,
    full_output=True)`` returns, which holds it under ``'full_output'``).  ``igauss``: as for ``_plane``."""
    full = x.get("full_output", x)
    for k in ("taugas", "taucld", "tauray"):
        if full.get(k) is None:
            raise Exception("contribution: the dictionary has no '%s' (spectrum(..., full_output=True)['full_output'])" % k)
    wno = np.asarray(full["wavenumber"], dtype=float)
    nlayer, nwno = len(full["layer"]["pressure"]), wno.size
    ctx = _lib.context()
    planes = [_plane(full[k], nlayer, nwno, ctx, igauss) for k in ("taugas", "taucld", "tauray")]
    return full, planes, wno, wno, ctx


def _check_case(opa, dimension, ck=False):
    if dimension != "1d":
        raise NotImplementedError("contribution functions: only dimension='1d' is supported")
    if opa is None:
        raise Exception("contribution: an inputs object needs the opacity object (opacityclass=)")
    if opa.ngauss > 1 and not ck:
        raise NotImplementedError(NO_CK)


def _case_planes(bundle, opa, dimension, ck=False):
    """``(atm, planes, wno, grid_of, ctx)`` of an ``inputs`` object: the atmosphere as ``get_contribution`` sets it up,
    TAUGAS / TAURAY from the gas stage and TAUCLD from the cloud tables, all three on the device (``taucld`` None: no
    cloud).  ``ck``: correlated-k tables are allowed and TAUGAS is then ``(nlayer, nwno, ngauss)``, the Gauss index fastest;
    TAURAY and TAUCLD have no Gauss axis.  Nothing that a later ``spectrum()`` reads is written: the plan's coefficient
    cache is left alone, as in ``optics.species_opacity``."""
    from .spectrum import _setup_atmosphere
    _check_case(opa, dimension, ck)
    inp = bundle.inputs
    atm = _setup_atmosphere(inp, opa, opa.wno)
    opa.get_opacities(atm, exclude_mol=inp["atmosphere"]["exclude_mol"])
    nlayer, nwno, ngauss, ctx = atm.c.nlayer, opa.nwno, opa.ngauss, opa.ctx
    taugas = DeviceArray((nlayer, nwno) if ngauss == 1 else (nlayer, nwno, ngauss), ctx)
    tauray = DeviceArray((nlayer, nwno), ctx)
    optics._gas_call(opa, nlayer, taugas=taugas, tauray=tauray, ngauss=ngauss,
                     **optics._gas_tables(opa, optics._layer_factors(atm, opa)))
    return atm, [taugas, optics._cloud_opd_device(atm, opa), tauray], opa.wno, opa, ctx


def _from_case(bundle, opa, dimension):
    """``_case_planes`` with the atmosphere as its ``full_output`` dictionary, as ``_from_dictionary`` returns it."""
    atm, planes, wno, grid_of, ctx = _case_planes(bundle, opa, dimension)
    return atm.as_dict(), planes, wno, grid_of, ctx


def _source(x, opacityclass, dimension):
    if isinstance(x, dict):
        if dimension != "1d":
            raise NotImplementedError("contribution functions: only dimension='1d' is supported")
        return _from_dictionary(x)
    return _from_case(x, opacityclass, dimension)


@_lib.serialized
def thermal_contribution(x, opacityclass=None, tau_max=1.0, R=100, dimension="1d"):
    """The emission contribution function of Lothringer+2018 eq. 4 as the reference evaluates it (justplotit.py:1584-1643):
    ``CF[l] = blackbody(T_l, 1/wno) * exp(-cumsum(t)[l]) * t[l] / diff(log(p_layer))[l]`` with ``t = taugas + taucld +
    tauray`` clipped at ``tau_max``, for the layers ``l = 0 .. nlayer-2`` (csrc/contribfn.hip: ``picaso_thermal_cf_dev``).

    ``x``: an ``inputs`` object (then ``opacityclass`` is required; the planes are formed on the device and none is copied
    to the host) or a ``full_output`` dictionary, the reference's calling form (its planes are uploaded).  Monochromatic
    opacities and ``dimension='1d'`` only.  Returns ``{'wavenumber', 'pressure', 'CF'}``: ``pressure`` = the layer
    pressures but the last [bar], ``CF`` ``(nlayer-1, n_out)``; with ``R`` every row is ``mean_regrid(wno, row,
    newx=wavenumber)``, ``wavenumber = mean_regrid(wno, wno, R=R)[0]``, bit for bit (binned on the device); ``R=None``:
    the native grid."""
    full, (taugas, taucld, tauray), wno, grid_of, ctx = _source(x, opacityclass, dimension)
    p_bar = np.asarray(full["layer"]["pressure"], dtype=float)
    tlayer = _lib.f64(full["layer"]["temperature"])
    nlayer, nwno = p_bar.size, int(np.size(wno))
    cf = DeviceArray((nlayer - 1, nwno), ctx) if nlayer > 1 else None
    if cf is not None:
        dlnp = _lib.f64(np.diff(np.log(p_bar)))
        d_wno = optics._wno_device(grid_of, wno) if grid_of is not wno else DeviceArray.from_host(wno, ctx)
        _lib.check(_lib.load().picaso_thermal_cf_dev(
            ctx, nlayer, nwno, nwno, _lib.ptr(taugas.addr),
            _lib.ptr(taucld.addr) if taucld is not None else None, _lib.ptr(tauray.addr), _lib.ptr(tlayer),
            _lib.ptr(d_wno.addr), _lib.ptr(dlnp), float(tau_max), _lib.ptr(cf.addr)), ctx)
        wavenumber, out = _binned(ctx, cf, wno, R, grid_of)
    else:
        wavenumber = wno if R is None else cf_grid(grid_of, R)[0]
        out = np.zeros((0, np.size(wavenumber)))
    return {"wavenumber": wavenumber, "pressure": p_bar[:-1], "CF": out}


@_lib.serialized
def transmission_contribution(x, opacityclass=None, R=None, as_reference=False, dimension="1d"):
    """The share of every layer in the transit depth, ``CF[k] = (norm - F_k) / sum_k (norm - F_k)`` with ``F_k`` the depth
    without layer ``k`` (reference justplotit.py:1697-1779), from one launch that sums non-negative terms
    (``picaso_transit_cf_dev``) instead of ``nlayer + 1`` transit depths and their differences.

    ``x``, ``opacityclass``, ``R``: as for ``thermal_contribution`` (``R`` defaults to None, as in the reference).  An
    ``inputs`` object needs ``gravity(radius=, mass=)`` for the altitudes.  By default the slant optical depths are those
    of ``spectrum('transmission')`` -- level pressures in dyn/cm^2, level temperatures, the real ``k_b`` and ``amu`` -- so
    the result describes the spectrum this package returns; ``as_reference=True`` passes what the reference's function
    passes (layer pressures in bar, layer temperatures, ``k_b = amu = 1``), which makes every slant optical depth about
    83 times larger (``1e-6 k_b / amu``) and is kept for parity only.  Returns ``{'wavenumber', 'pressure', 'CF'}``:
    ``pressure`` = the layer pressures [bar], ``CF`` ``(nlayer, n_out)``; a column that absorbs nothing is NaN."""
    if not isinstance(x, dict):
        _check_case(opacityclass, dimension)
        if np.isnan(x.inputs["planet"]["radius"]):
            raise Exception(NEEDS_RADIUS)
    full, (taugas, taucld, tauray), wno, grid_of, ctx = _source(x, opacityclass, dimension)
    level, layer = full["level"], full["layer"]
    z = level.get("z")
    if z is None or not np.all(np.isfinite(z)):
        raise Exception(NEEDS_RADIUS)
    p_bar = np.asarray(layer["pressure"], dtype=float)
    nlayer, nwno = p_bar.size, int(np.size(wno))
    nlevel = nlayer + 1
    if as_reference:                          # justplotit.py:1732-1738
        k_b = amu = 1.0
        player, tlayer = p_bar, layer["temperature"]
    else:                                     # justdoit.py:390-394
        k_b, amu = _Consts.k_b, _Consts.amu
        player, tlayer = np.asarray(level["pressure"], dtype=float) * _Consts.pconv, level["temperature"]
    # DTAU = (taugas + taucld) + tauray, as the reference adds its three planes (:1725-1727)
    dtau = DeviceArray((nlayer, nwno), ctx)
    if taucld is not None:
        resident.axpby(ctx, 1.0, taugas, 1.0, taucld, dtau)
        resident.axpby(ctx, 1.0, dtau, 1.0, tauray, dtau)
    else:
        resident.axpby(ctx, 1.0, taugas, 1.0, tauray, dtau)
    cf = DeviceArray((nlayer, nwno), ctx)
    _lib.check(_lib.load().picaso_transit_cf_dev(
        ctx, _lib.ptr(_lib.f64(z, (nlevel,))), _lib.ptr(_lib.f64(level["dz"], (nlevel,))), nlevel, nwno, nwno,
        1.0, _lib.ptr(_lib.f64(layer["mmw"], (nlayer,))), k_b, amu, _lib.ptr(_lib.f64(player)),
        _lib.ptr(_lib.f64(tlayer)), _lib.ptr(_lib.f64(layer["column_density"], (nlayer,))), _lib.ptr(dtau.addr),
        _lib.ptr(cf.addr)), ctx)
    wavenumber, out = _binned(ctx, cf, wno, R, grid_of)
    return {"wavenumber": wavenumber, "pressure": p_bar, "CF": out}
