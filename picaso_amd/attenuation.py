"""Where the photons stop, on the device: ``jdi.photon_attenuation``, ``jdi.taumap``, ``jdi.heatmap_taus`` and
``jdi.cloud_optics_1d``.

The remaining diagnostics of the reference that read the ``(nlayer, nwno)`` optical-depth planes ``taugas``, ``taucld``,
``tauray`` -- ``justplotit.photon_attenuation`` (justplotit.py:426-536), ``taumap`` (:1019-1131), ``heatmap_taus``
(:1284-1323) and the band means of ``all_optics_1d`` (:1197-1282) -- without their figures.  As in ``contribution.py``
every function takes an ``inputs`` object plus the opacity object (the planes are formed on the device and none is
copied to the host) or a ``full_output`` dictionary, the reference's calling form (its planes are uploaded); the same
kernels (csrc/attenuation.hip, and ``picaso_mean_regrid_plane_dev`` for the binning) serve both, and what comes back is
``nwno`` or ``nlayer x nbins`` numbers, not planes.
"""
import numpy as np

from . import _lib, optics, regrid
from .contribution import _binned, _case_planes, _from_dictionary, _plane
from .device import DeviceArray

COMPONENTS = ("gas", "cld", "ray")


def r_grid(opacityclass_or_wno, R):
    """``(wavenumber, plan)`` of ``mean_regrid(wno, row, R=R)``: the constant-``R`` bins themselves (``contribution.cf_grid``
    is the other form, bins half way between these centres)."""
    plan = regrid.regrid_plan(opacityclass_or_wno, R=R)
    return plan.centres, plan


def contiguous_window(wno, wave_range):
    """The columns with ``wave_range[0] < 1e4 / wno < wave_range[1]`` (justplotit.py:1261-1262) as ``(lo, hi)``, the
    half-open column range; ``(0, 0)`` when there is none.  Columns that do not follow one another: an exception."""
    wave = 1e4 / np.asarray(wno, dtype=float)
    inds = np.flatnonzero((wave > wave_range[0]) & (wave < wave_range[1]))
    if inds.size == 0:
        return 0, 0
    lo, hi = int(inds[0]), int(inds[-1]) + 1
    if hi - lo != inds.size:
        raise Exception("cloud_optics_1d: the columns of wave_range=%s are not contiguous on this wavenumber grid"
                        % (tuple(wave_range),))
    return lo, hi


def nearest_wavelength(wno, wavelength):
    """The column the reference's ``find_nearest_1d(1e4 / wno, wavelength)`` picks: the wavelength nearest to
    ``wavelength``, of two equally near ones the shorter (it sorts the wavelengths and keeps the first minimum)."""
    wave = 1e4 / np.asarray(wno, dtype=float)
    if np.unique(wave).size != wave.size:
        raise Exception("taumap: the wavenumber grid repeats a value")
    gap = np.abs(wave - wavelength)
    near = np.flatnonzero(gap == gap.min())
    return int(near[np.argmin(wave[near])])


def _tau_levels(ctx, nlayer, ncol, comps, plevel, at_tau, per_column=False, one_zero_is_bottom=False):
    """``picaso_tau_level_dev``.  ``comps``: for gas, cloud and Rayleigh ``(plane, (pitch, stride, offset), multiplier,
    (pitch, stride, offset))`` with DeviceArrays or None.  Returns ``(levels, pressure)``: an ``int32`` host array
    ``(4, ncol)`` -- the three level indices and the dominance code -- and the DeviceArray ``(3, ncol)`` of pressures."""
    planes = [c[0] for c in comps] + [c[2] for c in comps]
    layout = np.array([c[1] for c in comps] + [c[3] if c[3] is not None else (0, 1, 0) for c in comps], dtype=np.int64)
    table = _lib.ptr_array(planes)
    plev = _lib.f64(plevel)
    if plev.size != (ncol if per_column else 1) * (nlayer + 1):
        raise Exception("photon attenuation: %d level pressures for %d layers" % (plev.size, nlayer))
    levels = DeviceArray(((4 * ncol + 1) // 2,), ctx)              # int32, carried by a float64 buffer
    pressure = DeviceArray((3, ncol), ctx)
    _lib.check(_lib.load().picaso_tau_level_dev(
        ctx, nlayer, ncol, table, layout.ctypes.data, _lib.ptr(plev), 1 if per_column else 0, float(at_tau),
        1 if one_zero_is_bottom else 0, levels.addr, _lib.ptr(pressure.addr)), ctx)
    host = levels.to_host().view(np.int32)[:4 * ncol].reshape(4, ncol)      # waits for the launch: its inputs may go now
    return host, pressure


def _mono(nwno):
    return (nwno, 1, 0)


@_lib.serialized
def photon_attenuation(x, opacityclass=None, at_tau=0.5, igauss=0, R=None):
    """At which pressure the gas, the cloud (``taucld * w0``) and the Rayleigh optical depth each reach ``at_tau``, and which
    of them stops the photons first: the reference's ``justplotit.photon_attenuation(..., return_output=True)``
    (justplotit.py:426-536) without the figure, one launch of ``picaso_tau_level_dev`` (csrc/attenuation.hip).

    ``x``: an ``inputs`` object (then ``opacityclass`` is required; the planes are formed on the device and none is copied
    to the host) or a ``full_output`` dictionary (its planes are uploaded).  Correlated-k tables are supported in both
    forms: ``igauss`` selects the Gauss point (``igauss >= ngauss``: an exception).  Returns a dictionary with
    ``wavenumber``, ``wavelength`` [um], ``pressure_gas`` / ``pressure_cld`` / ``pressure_ray`` in the units of
    ``full_output['level']['pressure']`` [bar], ``level_gas`` / ``level_cld`` / ``level_ray`` (the level indices the
    reference's ``find_nearest_2d`` returns) and ``dominant``: 0 gas, 1 cloud, 2 Rayleigh where that pressure is strictly
    smaller than both others (the three masks of :509-511), -1 where none is.  A column that holds a NaN has level -1 and
    pressure NaN (the reference's answer there depends on the numpy version).  With ``R`` every pressure row
    is ``mean_regrid(wno, row, R=R)`` bit for bit, binned on the device; the levels and ``dominant`` are then omitted."""
    igauss = int(igauss)
    if igauss < 0:
        raise Exception("igauss=%d" % igauss)
    if isinstance(x, dict):
        full, (taugas, taucld, tauray), wno, grid_of, ctx = _from_dictionary(x, igauss)
        nlayer, nwno = taugas.shape
        w0 = _plane(full["layer"]["cloud"]["w0"], nlayer, nwno, ctx)
        plevel = np.asarray(full["level"]["pressure"], dtype=float)
        gas_layout = _mono(nwno)
    else:
        atm, (taugas, taucld, tauray), wno, grid_of, ctx = _case_planes(x, opacityclass, "1d", ck=True)
        ngauss, nlayer, nwno = opacityclass.ngauss, atm.c.nlayer, opacityclass.nwno
        if igauss >= ngauss:
            raise Exception("igauss=%d, but the opacity tables have %d Gauss point(s)" % (igauss, ngauss))
        w0 = optics._cloud_opd_device(atm, opacityclass, key="w0") if taucld is not None else None
        plevel = np.asarray(atm.level["pressure"], dtype=float) / atm.c.pconv
        gas_layout = (nwno * ngauss, ngauss, igauss)
    comps = [(taugas, gas_layout, None, None), (taucld, _mono(nwno), w0, _mono(nwno)), (tauray, _mono(nwno), None, None)]
    levels, pressure = _tau_levels(ctx, nlayer, nwno, comps, plevel, at_tau)
    wavenumber, p = _binned(ctx, pressure, wno, R, grid_of, grid=r_grid)
    out = {"wavenumber": wavenumber, "wavelength": 1e4 / np.asarray(wavenumber, dtype=float)}
    for i, k in enumerate(COMPONENTS):
        out["pressure_" + k] = p[i]
    if R is None:
        for i, k in enumerate(COMPONENTS):
            out["level_" + k] = levels[i].copy()
        out["dominant"] = levels[3].copy()
    return out


@_lib.serialized
def taumap(full_output, at_tau=1, wavelength=1, igauss=0):
    """The pressure at which every facet of a 3-D run reaches ``at_tau`` in gas, cloud (``taucld * w0``) and Rayleigh
    optical depth at the wavelength nearest to ``wavelength`` [um]: the maps of the reference's ``justplotit.taumap``
    (justplotit.py:1019-1131) without the globes.  ``full_output``: the dictionary of a 3-D run -- ``taugas`` / ``taucld`` /
    ``tauray`` ``(nlayer, nwno, ng, nt, ngauss)``, the cloud ``w0`` ``(nlayer, nwno, ng, nt)``, level pressures ``(nlevel,
    ng, nt)``.  The ``ng * nt`` facet columns go through ``picaso_tau_level_dev`` with their own level pressures.  Returns
    ``map_gas``, ``map_cld``, ``map_ray`` ``(ng, nt)``, ``latitude``, ``longitude``.

    Quirk, reproduced as the reference writes it (:1082-1083): when the cumulative cloud column of a facet holds exactly
    one zero -- its top, so the cloud is non-zero in the first layer -- the cloud level becomes ``nlayer``, the bottom of
    the atmosphere, whatever ``at_tau`` is.  (The test was presumably meant to catch a column of zeros.)"""
    full = full_output.get("full_output", full_output)
    igauss = int(igauss)
    planes = [np.asarray(full[k], dtype=float) for k in ("taugas", "taucld", "tauray")]
    if any(a.ndim != 5 for a in planes):
        raise Exception("taumap: the dictionary of a 3-D run is needed (planes of shape (nlayer, nwno, ng, nt, ngauss))")
    nlayer, nwno, ng, nt, ngauss = planes[0].shape
    if not 0 <= igauss < ngauss:
        raise Exception("igauss=%d, but the planes hold %d Gauss point(s)" % (igauss, ngauss))
    iw = nearest_wavelength(full["wavenumber"], wavelength)
    nfac = ng * nt
    ctx = _lib.context()
    # the facet columns of wavelength iw, Gauss point still fastest: element (l, f) at l * nfac * ngauss + f * ngauss + igauss
    dev = [DeviceArray.from_host(np.ascontiguousarray(a[:, iw]).reshape(nlayer, nfac * ngauss), ctx) for a in planes]
    w0 = np.asarray(full["layer"]["cloud"]["w0"], dtype=float)
    if w0.shape != (nlayer, nwno, ng, nt):
        raise Exception("taumap: the cloud w0 has shape %s, expected %s" % (w0.shape, (nlayer, nwno, ng, nt)))
    d_w0 = DeviceArray.from_host(np.ascontiguousarray(w0[:, iw]).reshape(nlayer, nfac), ctx)
    plevel = np.asarray(full["level"]["pressure"], dtype=float)
    if plevel.shape != (nlayer + 1, ng, nt):
        raise Exception("taumap: level pressures of shape %s, expected %s" % (plevel.shape, (nlayer + 1, ng, nt)))
    sets = np.ascontiguousarray(plevel.reshape(nlayer + 1, nfac).T)          # (facet, level)
    lay = (nfac * ngauss, ngauss, igauss)
    comps = [(dev[0], lay, None, None), (dev[1], lay, d_w0, (nfac, 1, 0)), (dev[2], lay, None, None)]
    _, pressure = _tau_levels(ctx, nlayer, nfac, comps, sets, at_tau, per_column=True, one_zero_is_bottom=True)
    p = pressure.to_host().reshape(3, ng, nt)
    return {"map_gas": p[0], "map_cld": p[1], "map_ray": p[2],
            "latitude": full.get("latitude"), "longitude": full.get("longitude")}


def _log10(a):
    """justplotit.py:1309-1310 on the small array that came back: zeros become 1e-100, then numpy's own log10."""
    a = np.array(a, dtype=float)
    a[a == 0] = 1e-100
    with np.errstate(all="ignore"):
        return np.log10(a)


@_lib.serialized
def heatmap_taus(x, opacityclass=None, R=0):
    """The three optical-depth planes as ``log10`` over (layer pressure, wavenumber): the ``Z`` arrays of the reference's
    ``justplotit.heatmap_taus`` (justplotit.py:1284-1323) at Gauss point 0, without the figure.

    ``x``: an ``inputs`` object (with ``opacityclass``; monochromatic opacities) or the dictionary of ``spectrum(...,
    full_output=True)`` / a ``full_output`` dictionary.  With ``R > 0`` every layer row is binned with ``mean_regrid(wno,
    row, R=R)`` on the device and only ``(nlayer, nbins)`` per plane comes back (an empty bin is NaN); ``R = 0``: the
    planes come back unbinned, as the reference returns them.  The replacement of zeros by ``1e-100`` and ``np.log10`` run
    on the host on what came back, so the values are numpy's own.  Returns ``wavenumber``, ``pressure`` (layer) and
    ``taugas``, ``taucld``, ``tauray``."""
    if isinstance(x, dict):
        full, planes, wno, grid_of, ctx = _from_dictionary(x, 0)
        pressure = np.asarray(full["layer"]["pressure"], dtype=float)
    else:
        if opacityclass is not None and opacityclass.ngauss > 1:
            raise NotImplementedError("heatmap_taus of an inputs object: monochromatic opacities only (binning one Gauss "
                                      "point of a resident correlated-k plane is not implemented; pass the full_output "
                                      "dictionary)")
        atm, planes, wno, grid_of, ctx = _case_planes(x, opacityclass, "1d")
        pressure = np.asarray(atm.layer["pressure"], dtype=float) / atm.c.pconv
        if planes[1] is None:                                  # no cloud: a plane of zeros, -100 after the logarithm
            planes[1] = DeviceArray.zeros(planes[0].shape, ctx)
    out = {"pressure": pressure}
    for k, plane in zip(("taugas", "taucld", "tauray"), planes):
        out["wavenumber"], a = _binned(ctx, plane, wno, R if R else None, grid_of, grid=r_grid)
        out[k] = _log10(a)
    return {k: out[k] for k in ("wavenumber", "pressure", "taugas", "taucld", "tauray")}


@_lib.serialized
def cloud_optics_1d(x, opacityclass=None, wave_range=(0.3, 1.0), ng=None, nt=None):
    """The cloud's optical depth per layer, single-scattering albedo and asymmetry averaged over the wavelengths with
    ``wave_range[0] < 1e4 / wno < wave_range[1]`` [um]: the profiles the reference's ``justplotit.all_optics_1d``
    (justplotit.py:1197-1282) draws, by ``picaso_band_mean_rows_dev`` in one launch.

    ``x``: an ``inputs`` object (with ``opacityclass``; the cloud tables are formed on the device) or a ``full_output``
    dictionary; ``ng``, ``nt`` select one facet of a 3-D dictionary on the host.  The window is found on the host and must
    be contiguous; an empty window gives NaN, as ``np.mean`` of an empty slice.  The sums differ from numpy's pairwise
    ones in their order alone: both lie within ``(n - 1) 2^-53 sum|x|`` of the exact sum over the ``n`` columns.  Returns
    ``pressure`` (layer), ``opd``, ``w0``, ``g0``, each ``(nlayer,)``."""
    if (ng is None) != (nt is None):
        raise Exception("cloud_optics_1d: give both ng and nt, or neither")
    if isinstance(x, dict):
        full = x.get("full_output", x)
        wno = np.asarray(full["wavenumber"], dtype=float)
        cloud = full["layer"]["cloud"]
        pressure = np.asarray(full["layer"]["pressure"], dtype=float)
        tabs = [np.asarray(cloud[k], dtype=float) for k in ("opd", "w0", "g0")]
        if ng is not None:
            pressure, tabs = pressure[:, ng, nt], [t[:, :, ng, nt] for t in tabs]
        nlayer, nwno = pressure.size, wno.size
        ctx = _lib.context()
        planes = [_plane(t, nlayer, nwno, ctx) for t in tabs]
    else:
        if ng is not None:
            raise NotImplementedError("cloud_optics_1d: ng, nt select a facet of a 3-D full_output dictionary")
        atm, _, wno, _, ctx = _case_planes(x, opacityclass, "1d", ck=True)
        nlayer, nwno = atm.c.nlayer, opacityclass.nwno
        pressure = np.asarray(atm.layer["pressure"], dtype=float) / atm.c.pconv
        planes = [optics._cloud_opd_device(atm, opacityclass, key=k) for k in ("opd", "w0", "g0")]
        if planes[0] is None:                                  # no cloud: the reference's tables are zeros
            planes = [DeviceArray.zeros((nlayer, nwno), ctx)] * 3
    lo, hi = contiguous_window(wno, wave_range)
    means = DeviceArray((3, nlayer), ctx)
    _lib.check(_lib.load().picaso_band_mean_rows_dev(
        ctx, nlayer, nwno, nwno, lo, hi, 3, *[_lib.ptr(p.addr) for p in planes], _lib.ptr(means.addr)), ctx)
    m = means.to_host()
    return {"pressure": pressure, "opd": m[0], "w0": m[1], "g0": m[2]}
