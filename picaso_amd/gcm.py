"""A GCM cloud map resident in HBM and the cloud tables of every phase of a phase curve regridded from it in one launch
(``inputs.clouds_4d``; reference justdoit.py:3875-4090).

The host regrid (``justdoit._regrid_lonlat``) interpolates the whole map -- ``opd``, ``w0``, ``g0`` on
``(lon, lat, pressure, wno)`` -- along longitude and latitude per phase, and the spectrum then re-stacks, fingerprints and
uploads the result.  What a phase needs from the map is four neighbouring columns per facet: here the map goes to HBM once
(``GcmCloudMap``), the searches stay on the host as index tables of ``nphase * (ng + nt)`` entries
(``spectrum._axis_indices``, the index form of ``_interp_axis``), and ``picaso_gcm_facet_tables_dev`` writes the
``(3, nfacets * nlayer, nin)`` rows of every phase where the fused opacity launch reads them (``FacetCloudTables``).
"""
import os

import numpy as np

from . import _lib, device
from .chemistry import _upload_i32
from .device import DeviceArray
from .spectrum import _axis_indices, _lon_period

_VARS = ("opd", "w0", "g0")

_maps = {}              # (pid, context, digest of the map) -> GcmCloudMap: content-addressed, oldest out first
_MAPS_MAX = 2           # (a native map is 2 GB)
UPLOADS = 0             # maps uploaded by this process so far (a memo hit does not count)
_lib.on_context_destroy(lambda value: [_maps.pop(k) for k in [k for k in _maps if k[1] == value]])


def clear_map_cache():
    """Drop the resident cloud maps kept by ``GcmCloudMap.resident``."""
    _maps.clear()


class GcmCloudMap(object):
    """``opd``, ``w0`` and ``g0`` of a GCM cloud map in HBM, each ``(nlon, nlat, npres, nin)`` in the caller's own order
    along every axis, with the coordinates ``lon`` / ``lat`` (degrees), ``pressure`` (bar) and ``wno`` and the two
    permutations the regrid launch applies: ``layer_src`` (pressure ascending: layers top to bottom) and ``wno_src``
    (wavenumber increasing), both as ``clouds_3d`` sorts them.

    ``GcmCloudMap.resident(coords, variables, ctx)`` memoises by content: the same arrays are uploaded once per context."""

    def __init__(self, coords, variables, ctx=None, digest=None):
        global UPLOADS
        self.ctx = ctx if ctx is not None else _lib.context()
        self.lon, self.lat, self.pressure, self.wno = (np.asarray(coords[k], dtype=float).reshape(-1)
                                                       for k in ("lon", "lat", "pressure", "wno"))
        shape = (self.lon.size, self.lat.size, self.pressure.size, self.wno.size)
        if min(shape) < 1:
            raise ValueError("cloud map: an empty coordinate (lon, lat, pressure, wno have %s points)" % (shape,))
        for k in _VARS:
            if np.shape(variables[k]) != shape:
                raise ValueError("cloud map: %s has shape %s, its coordinates (lon, lat, pressure, wno) give %s"
                                 % (k, np.shape(variables[k]), shape))
        self.shape = shape
        self.layer_src = np.argsort(self.pressure)
        self.wno_src = np.argsort(self.wno)
        self.pressure_sorted = self.pressure[self.layer_src]
        self.wno_sorted = np.ascontiguousarray(self.wno[self.wno_src])
        self.digest = digest if digest is not None else _map_digest(coords, variables)
        self.device = _lib.device_of(self.ctx)
        self.d_vars = [DeviceArray.from_host(variables[k], self.ctx) for k in _VARS]
        self.d_wno = DeviceArray.from_host(self.wno_sorted, self.ctx)
        self.d_perm = _upload_i32(np.concatenate([self.layer_src, self.wno_src]), self.ctx)
        self.nbytes = sum(d.nbytes for d in self.d_vars)
        UPLOADS += 1

    @classmethod
    def resident(cls, coords, variables, ctx=None):
        """The resident form of the map ``(coords, variables)`` (what ``justdoit._dataset_like`` returns), from the memo
        when a map of the same content is already in HBM on this context."""
        ctx = ctx if ctx is not None else _lib.context()
        digest = _map_digest(coords, variables)
        key = (os.getpid(), getattr(ctx, "value", ctx), digest)
        hit = _maps.get(key)
        if hit is None:
            while len(_maps) >= _MAPS_MAX:
                del _maps[next(iter(_maps))]
            hit = _maps[key] = cls(coords, variables, ctx, digest)
        return hit

    def rotated_lon(self, rotation):
        """The map's longitudes as a phase sees them: every term of ``rotation`` (a number, or a sequence added left to
        right -- ``atmosphere_4d`` adds the phase in degrees, then the shift) added, wrapped to [-180, 180)."""
        lon = self.lon
        for r in np.atleast_1d(rotation):
            lon = lon + r
        return (lon + 180.0) % 360.0 - 180.0


def _map_digest(coords, variables):
    from .optics import content_digest
    return tuple(content_digest(np.asarray(a, dtype=np.float64))
                 for a in [variables[k] for k in _VARS] + [coords[k] for k in ("lon", "lat", "pressure", "wno")])


def phase_index_tables(cmap, lon_facets, lat_facets, rotation):
    """``(j0, j1, t), (i0, i1, u)`` of one phase: the source columns and weights of ``lon_facets`` on the map's rotated
    longitudes (periodic when the map goes round the planet: ``spectrum._lon_period``, the test of ``_regrid_lonlat``) and
    of ``lat_facets`` on its latitudes, all as indices into the map's own axes."""
    lon_rot = cmap.rotated_lon(rotation)
    return (_axis_indices(lon_facets, lon_rot, period=_lon_period(lon_rot)), _axis_indices(lat_facets, cmap.lat))


@_lib.serialized
def facet_tables(cmap, lon_facets, lat_facets, rotations):
    """The cloud tables of every phase in ONE launch (``picaso_gcm_facet_tables_dev``): ``lon_facets[i]`` (``ng`` Gauss
    longitudes) and ``lat_facets[i]`` (``nt`` Chebyshev latitudes) are the facets of phase ``i`` in degrees,
    ``rotations[i]`` what is added to the map's longitudes for it (``GcmCloudMap.rotated_lon``).  Bilinear, longitude first
    and latitude second, with the bits of ``justdoit._regrid_lonlat``; no interpolation in pressure.  Returns one
    ``FacetCloudTables`` per phase, all views of one ``(nphase, 3, ng * nt * nlayer, nin)`` device array."""
    nphase = len(rotations)
    if len(lon_facets) != nphase or len(lat_facets) != nphase:
        raise ValueError("facet_tables: %d rotations, %d longitude sets, %d latitude sets"
                         % (nphase, len(lon_facets), len(lat_facets)))
    if nphase == 0:
        return []
    lon_facets = [np.asarray(x, dtype=float).reshape(-1) for x in lon_facets]
    lat_facets = [np.asarray(x, dtype=float).reshape(-1) for x in lat_facets]
    ng, nt = lon_facets[0].size, lat_facets[0].size
    if any(x.size != ng for x in lon_facets) or any(x.size != nt for x in lat_facets) or ng < 1 or nt < 1:
        raise ValueError("facet_tables: every phase needs the same number of Gauss and Chebyshev angles")
    nlon, nlat, npres, nin = cmap.shape
    lon_idx, lat_idx = np.empty((nphase, ng, 2), dtype=np.int32), np.empty((nphase, nt, 2), dtype=np.int32)
    lon_t, lat_u = np.empty((nphase, ng)), np.empty((nphase, nt))
    for i in range(nphase):
        (j0, j1, t), (i0, i1, u) = phase_index_tables(cmap, lon_facets[i], lat_facets[i], rotations[i])
        lon_idx[i, :, 0], lon_idx[i, :, 1], lon_t[i] = j0, j1, t
        lat_idx[i, :, 0], lat_idx[i, :, 1], lat_u[i] = i0, i1, u
    # the kernel clamps; a table that would need it is refused here
    if lon_idx.min() < 0 or lon_idx.max() >= nlon or lat_idx.min() < 0 or lat_idx.max() >= nlat:
        raise _lib.PicasoHipError("facet_tables: an index table points outside the map")
    if not (np.all(np.isfinite(lon_t)) and np.all(np.isfinite(lat_u))):
        raise _lib.PicasoHipError("facet_tables: a weight is not finite (coordinates with NaN?)")
    ctx = cmap.ctx
    nlayer = npres
    d_idx = _upload_i32(np.concatenate([lon_idx.ravel(), lat_idx.ravel()]), ctx)
    d_wts = DeviceArray.from_host(np.concatenate([lon_t.ravel(), lat_u.ravel()]), ctx)
    out = DeviceArray((nphase, 3, ng * nt * nlayer, nin), ctx)
    _lib.check(_lib.load().picaso_gcm_facet_tables_dev(
        ctx, nlon, nlat, npres, nin, cmap.d_vars[0].addr, cmap.d_vars[1].addr, cmap.d_vars[2].addr, nphase, ng, nt, nlayer,
        d_idx.addr, d_wts.addr, d_idx.addr + 4 * lon_idx.size, d_wts.addr + 8 * lon_t.size, cmap.d_perm.addr,
        cmap.d_perm.addr + 4 * npres, out.addr), ctx)
    # the tables are read from other contexts' streams of this device (an opacity object's, a replica's): written before
    # anyone can ask for them.  One wait per clouds_4d, not per phase; it also covers the index uploads going out of scope
    device.sync(ctx)
    from .optics import content_digest
    return [FacetCloudTables(cmap, out.row_block(i), ng, nt,
                             (cmap.digest, tuple(float(r) for r in np.atleast_1d(rotations[i])),
                              content_digest(lon_facets[i]), content_digest(lat_facets[i])))
            for i in range(nphase)]


class FacetCloudTables(dict):
    """The cloud tables of one phase, made in HBM by ``facet_tables``: what ``inputs['clouds']['profile_3d']`` may hold in
    place of the dictionary ``clouds_3d`` stores.  Two faces:

    * ``resident_tables(nlayer, nfacets, ctx)``: the ``(d_xp, d_tall, None, nin)`` of ``optics._facet_major_cloud_tables``
      for a context on the map's device -- the rows where they lie, no host copy (``None`` stands for the host rows), no
      fingerprint (``stamp``: the map's digest, the phase's rotation and the facet grid), no upload.  ``None`` for a
      context on another device or another shape: the caller goes on with the dictionary face.
    * a dictionary: ``wavenumber`` (increasing) and ``pressure`` (layers top to bottom) are plain entries; ``opd``, ``w0``,
      ``g0`` appear on first use as ``(nlayer, nin, ng, nt)`` host arrays, by one copy back -- the dictionary ``clouds_3d``
      would have stored, bit for bit, and from then on every consumer treats it as that.  ``materialized`` says whether
      that has happened.

    The object is not meant to be edited; a deep copy is the object itself, a pickle is the plain host dictionary."""

    def __init__(self, cmap, d_tall, ng, nt, stamp):
        dict.__init__(self, wavenumber=cmap.wno_sorted, pressure=cmap.pressure_sorted)
        self.map, self.d_tall, self.ng, self.nt, self.stamp = cmap, d_tall, int(ng), int(nt), stamp
        self.nlayer, self.nin = cmap.shape[2], cmap.shape[3]
        self.materialized = False

    # ---- the resident face
    def resident_tables(self, nlayer, nfac, ctx):
        if nlayer != self.nlayer or nfac != self.ng * self.nt or self.nin < 2:
            return None
        if getattr(ctx, "value", ctx) != getattr(self.map.ctx, "value", self.map.ctx) \
                and _lib.device_of(ctx) != self.map.device:
            return None
        return self.map.d_wno, self.d_tall, None, self.nin

    # ---- the dictionary face
    def _fill(self):
        if self.materialized:
            return
        host = self.d_tall.to_host().reshape(3, self.ng, self.nt, self.nlayer, self.nin)
        tail = {k: dict.pop(self, k) for k in ("wavenumber", "pressure")}
        for k, a in zip(_VARS, host):                   # (ng, nt, nlayer, nin) -> (nlayer, nin, ng, nt), as clouds_3d stores it
            dict.__setitem__(self, k, np.ascontiguousarray(np.transpose(a, (2, 3, 0, 1))))
        dict.update(self, tail)
        self.materialized = True

    def __getitem__(self, key):
        if key in _VARS:
            self._fill()
        return dict.__getitem__(self, key)

    def get(self, key, default=None):
        if key in _VARS:
            self._fill()
        return dict.get(self, key, default)

    def __contains__(self, key):
        return key in _VARS or dict.__contains__(self, key)

    def __len__(self):
        return dict.__len__(self) + (0 if self.materialized else len(_VARS))

    def __iter__(self):
        self._fill()
        return dict.__iter__(self)

    def keys(self):
        self._fill()
        return dict.keys(self)

    def items(self):
        self._fill()
        return dict.items(self)

    def values(self):
        self._fill()
        return dict.values(self)

    def copy(self):
        return dict(self.items())

    def __deepcopy__(self, memo):
        return self

    __copy__ = lambda self: self

    def __reduce__(self):
        return dict, (dict(self.items()),)
