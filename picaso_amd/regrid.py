"""Spectra binned to an instrument grid on the device: ``spectrum(regrid=...)``.

A retrieval compares binned spectra with data: after every forward model the reference's callers run ``mean_regrid``
(justplotit.py:31-63) over each spectral array -- on the host, 5-6 ms per array at 1e5 wavelengths, ten times the
spectrum it follows, plus the copies of the full-resolution arrays.  Here the bins are found once per wavenumber grid
(``RegridPlan``: bin ``j`` is the contiguous column range ``[start[j], start[j + 1])``), the means are formed on the
device behind the solvers (``picaso_mean_regrid_dev``, csrc/regrid.hip) together with the flux ratios of the output
dictionary, and ``nbins`` doubles per output come back.  The sums are taken in ``np.bincount``'s order, so every binned
array is bit for bit ``jdi.mean_regrid`` of the array the plain call returns.
"""
import ctypes
import weakref

import numpy as np

from . import _lib, device
from .device import DeviceArray

MAX_ROWS = 8            # PICASO_REGRID_MAX_ROWS
_plans = weakref.WeakSet()


class _Row(ctypes.Structure):
    """``picaso_regrid_row``"""
    _fields_ = [("op", ctypes.c_int), ("a", ctypes.c_void_p), ("b", ctypes.c_void_p), ("c", ctypes.c_void_p),
                ("k1", ctypes.c_double), ("k2", ctypes.c_double)]


class Reduction:
    """What ``spectrum(regrid=...)`` and ``spectrum(convolve=...)`` share: a plan on one wavenumber grid that turns the
    resident spectral arrays of a call into ``nout`` values per array behind the legs.  A plan gives ``nout``,
    ``out_wavenumber`` (the ``wavenumber`` of the output dictionary), ``counts`` (stored under ``counts_key``), ``kind``
    (the keyword, for messages) and ``launch(ctx, nrows, crows, out_addr)``, which enqueues its kernel and returns the
    device tables the launch reads."""

    def enqueue(self, ctx, rows, tails=(), keep=None):
        """One launch and one small copy on ``ctx``'s stream (``Binned``): the hook of ``onecall.enqueue_regrid`` and
        ``Spectrum._enqueue_regrid``."""
        return Binned(self, ctx, rows, tails, keep)

    def output(self, vals, lists, bond_albedo=None, effective_temperature=None):
        return output(self, vals, lists, bond_albedo, effective_temperature)

    def empty_output(self):
        """The dictionary of a call that names no leg."""
        return {"wavenumber": self.out_wavenumber, self.counts_key: self.counts}

    def check_grid(self, opa):
        if self.nwno != opa.nwno or not (self.wno is opa.wno or np.array_equal(self.wno, opa.wno)):
            raise Exception("%s: the plan was made for another wavenumber grid than the opacity object's" % self.kind)
        return self


class RegridPlan(Reduction):
    """The bins of one wavenumber grid: ``edges`` (nbins + 1), ``centres``, ``counts`` (points per bin), ``start`` (the
    first column of every bin and, last, the end of the last one) with ``mean_regrid``'s semantics -- bins are
    ``[e_j, e_j+1)``, the last one includes its right edge, columns outside all edges belong to no bin.  ``start`` is
    uploaded once per context, when a spectrum first uses the plan."""
    kind, counts_key = "regrid", "regrid_counts"
    nout = property(lambda self: self.nbins)
    out_wavenumber = property(lambda self: self.centres)

    def __init__(self, wno, newx=None, R=None):
        from .justdoit import create_grid
        x = np.asarray(wno, dtype=float)
        if x.ndim != 1 or x.size < 1:
            raise Exception("regrid_plan: the wavenumber grid must be a non-empty 1-D array")
        if np.any(np.diff(x) <= 0):
            raise Exception("regrid_plan: the wavenumber grid must be increasing")
        if newx is None and R is not None:
            edges = create_grid(1e4 / np.max(x), 1e4 / np.min(x), R)
        elif newx is not None and R is None:
            newx = np.asarray(newx, dtype=float)
            if newx.ndim != 1 or newx.size < 2:
                raise Exception("regrid_plan: newx must hold at least two points")
            d = np.diff(newx)
            if np.any(d <= 0):
                raise Exception("regrid_plan: newx must be strictly increasing")
            edges = np.concatenate(([newx[0] - d[0] / 2], newx[:-1] + d / 2.0, [newx[-1] + d[-1] / 2]))
        else:
            raise Exception("Please either enter a newx or a R")
        nb = edges.size - 1
        if nb < 1:
            raise Exception("regrid_plan: the new grid has no bins")
        start = np.empty(nb + 1, dtype=np.int64)
        start[:nb] = np.searchsorted(x, edges[:nb], side="left")          # the first x >= e_j
        start[nb] = np.searchsorted(x, edges[nb], side="right")           # the last bin is closed: x <= e_nbins
        np.maximum.accumulate(start, out=start)
        self.wno, self.nwno, self.nbins = wno, int(x.size), int(nb)
        self.edges = edges
        self.centres = (edges[:-1] + edges[1:]) / 2.0
        self.start = start.astype(np.int32)
        self.counts = np.diff(start)
        for a in (self.edges, self.centres, self.start, self.counts):
            a.flags.writeable = False
        self._dev = {}
        _plans.add(self)

    def device_start(self, ctx):
        """``start`` in HBM on ``ctx``'s device (int32; carried by a float64 DeviceArray of the same bytes)."""
        key = getattr(ctx, "value", ctx)
        hit = self._dev.get(key)
        if hit is None:
            padded = np.zeros((self.nbins + 2) // 2 * 2, dtype=np.int32)
            padded[:self.nbins + 1] = self.start
            hit = self._dev[key] = DeviceArray.from_host(padded.view(np.float64), ctx)
        return hit

    def launch(self, ctx, nrows, crows, out_addr):
        d_start = self.device_start(ctx)
        _lib.check(_lib.load().picaso_mean_regrid_dev(ctx, self.nwno, self.nbins, d_start.addr, nrows, crows, out_addr), ctx)
        return d_start


def _drop_context(value):
    """``destroy_context``: a new context may be created at the same address later."""
    for plan in list(_plans):
        plan._dev.pop(value, None)


_lib.on_context_destroy(_drop_context)


def regrid_plan(opacityclass_or_wno, newx=None, R=None):
    """The ``RegridPlan`` of a wavenumber grid (an opacity object, or the array itself) for ``newx`` (bin edges half way
    between its points) or constant resolution ``R`` -- ``mean_regrid``'s two forms, one of which must be given.  With an
    opacity object the plan is kept on it by content: equal ``R`` or equal ``newx`` values give the same plan again, and its
    bin table is uploaded once."""
    wno = getattr(opacityclass_or_wno, "wno", None)
    if wno is None:
        return RegridPlan(opacityclass_or_wno, newx=newx, R=R)
    if (newx is None) == (R is None):
        raise Exception("Please either enter a newx or a R")
    opa = opacityclass_or_wno
    if R is not None:
        key = ("R", float(R))
    else:
        a = np.ascontiguousarray(newx, dtype=float)
        key = ("newx", a.shape, a.tobytes())
    cache = opa.__dict__.setdefault("_regrid_plans", {})
    hit = cache.get(key)
    if hit is None or hit.wno is not wno:
        if len(cache) > 16:
            cache.clear()
        hit = cache[key] = RegridPlan(wno, newx=newx, R=R)
    return hit


def resolve(regrid, opa):
    """``regrid=`` of the public calls -> a plan on ``opa``'s grid: a ``RegridPlan``, ``{'R': r}`` or ``{'newx': array}``."""
    if isinstance(regrid, RegridPlan):
        return regrid.check_grid(opa)
    if isinstance(regrid, dict) and set(regrid) <= {"R", "newx"}:
        return regrid_plan(opa, newx=regrid.get("newx"), R=regrid.get("R"))
    raise Exception("regrid must be a regrid_plan(), {'R': r} or {'newx': array}")


class InstrumentsPlan(Reduction):
    """Several instruments on one wavenumber grid: the points of its members -- a ``RegridPlan`` (bin means) or a
    ``ConvolvePlan`` (Gaussian windows) each, with their own host tables, unchanged -- concatenated in the given order, for
    ONE call of ``picaso_instruments_reduce_dev`` (csrc/instruments.hip) behind the legs: the reference's loop over
    ``observation_data`` (driver.py:232-236) without a second spectrum and without the full-resolution copies.

    ``members`` (``{name: plan}``), ``slices`` (``{name: slice}`` into every output array), ``nout`` (the sum),
    ``out_wavenumber`` and ``counts`` (the members', concatenated), and per point in instrument order ``lo``, ``hi`` (int32),
    ``centre``, ``den`` (0.0 at a mean point, which reads neither).  The device tables hold the same points with the mean
    points first: device point ``p`` is instrument point ``col[p]``, ``nmean`` of them are means, ``ngauss`` Gaussian.
    ``scale``: every column of EVERY row of the call is multiplied by it before it is summed (one rounded product), as the
    reference scales the flux before it bins it (driver.py:230) -- the flux ratios of a planet (``fpfs_*``), ``albedo``
    and ``transit_depth`` included, so a scale belongs to a call that reads ``thermal`` alone, as ``retrieve.MODEL``'s; ``with_scale(k)`` gives the same plan, tables shared, with another scale."""
    kind, counts_key = "instruments", "instrument_counts"

    def __init__(self, wno, members, scale=1.0):
        if not members:
            raise Exception("instruments_plan: at least one instrument is needed")
        self.members = dict(members)
        lo, hi, centre, den, is_mean, self.slices = [], [], [], [], [], {}
        n0 = 0
        for name, m in self.members.items():
            if isinstance(m, RegridPlan):
                lo.append(m.start[:-1]), hi.append(m.start[1:])
                centre.append(np.zeros(m.nout)), den.append(np.zeros(m.nout))
            elif m.kind == "convolve":
                lo.append(m.lo), hi.append(m.hi), centre.append(m.centre), den.append(m.den)
            else:
                raise Exception("instruments_plan: instrument %r is neither a regrid nor a convolve plan" % (name,))
            is_mean.append(np.full(m.nout, isinstance(m, RegridPlan)))
            self.slices[name] = slice(n0, n0 + m.nout)
            n0 += m.nout
        first = next(iter(self.members.values()))
        self.wno, self.nwno, self.nout = wno, first.nwno, n0
        self.lo, self.hi = np.concatenate(lo).astype(np.int32), np.concatenate(hi).astype(np.int32)
        self.centre, self.den = np.concatenate(centre).astype(float), np.concatenate(den).astype(float)
        is_mean = np.concatenate(is_mean)
        self.col = np.concatenate((np.flatnonzero(is_mean), np.flatnonzero(~is_mean))).astype(np.int32)
        self.nmean, self.ngauss = int(is_mean.sum()), int((~is_mean).sum())
        self.out_wavenumber = np.concatenate([m.out_wavenumber for m in self.members.values()])
        self.counts = np.concatenate([np.asarray(m.counts, dtype=np.int64) for m in self.members.values()])
        for a in (self.lo, self.hi, self.centre, self.den, self.col, self.out_wavenumber, self.counts):
            a.flags.writeable = False
        self.scale = float(scale)
        self._dev = {}
        self._siblings = {}                             # scale -> plan, shared by every sibling (with_scale)
        _plans.add(self)

    def with_scale(self, scale):
        """This plan with another ``scale``.  The sibling shares the host tables, the device tables (``_dev``, which
        ``destroy_context`` empties through any of them: every sibling is registered) and the record of siblings already
        made, so equal scales give the same object again."""
        scale = float(scale)
        if scale == self.scale:
            return self
        import copy
        other = self._siblings.get(scale)
        if other is None:
            if len(self._siblings) > 64:
                self._siblings.clear()
            other = self._siblings[scale] = copy.copy(self)      # shallow: _dev and _siblings are the same objects
            other.scale = scale
            _plans.add(other)
        return other

    def device_tables(self, ctx):
        """``(ints, doubles, model_wl)`` in HBM on ``ctx``'s device, in device order: ``ints`` holds ``lo``, ``hi``, ``col``
        (int32, carried by a float64 DeviceArray of the same bytes), ``doubles`` holds ``centre`` then ``den``, ``model_wl``
        is the first Gaussian member's (None without one)."""
        key = getattr(ctx, "value", ctx)
        hit = self._dev.get(key)
        if hit is None:
            n = self.nout
            ints = np.zeros((3 * n + 1) // 2 * 2, dtype=np.int32)
            ints[:n], ints[n:2 * n], ints[2 * n:3 * n] = self.lo[self.col], self.hi[self.col], self.col
            dbl = np.concatenate((self.centre[self.col], self.den[self.col]))
            wl = next((m.device_tables(ctx)[0] for m in self.members.values() if m.kind == "convolve"), None)
            hit = self._dev[key] = (DeviceArray.from_host(ints.view(np.float64), ctx), DeviceArray.from_host(dbl, ctx), wl)
        return hit

    def launch(self, ctx, nrows, crows, out_addr):
        tables = d_int, d_dbl, d_wl = self.device_tables(ctx)
        n = self.nout
        _lib.check(_lib.load().picaso_instruments_reduce_dev(
            ctx, self.nwno, _lib.addr(d_wl), self.nmean, self.ngauss, d_int.addr, d_int.addr + 4 * n, d_int.addr + 8 * n,
            d_dbl.addr, d_dbl.addr + 8 * n, self.scale, nrows, crows, out_addr), ctx)
        return tables

    def output(self, vals, lists, bond_albedo=None, effective_temperature=None):
        out = output(self, vals, lists, bond_albedo, effective_temperature)
        out["instrument_slices"] = dict(self.slices)
        return out

    def empty_output(self):
        return dict(Reduction.empty_output(self), instrument_slices=dict(self.slices))


def _member_key(spec):
    if not isinstance(spec, dict) or not spec or not (set(spec) <= {"newx", "R"} or set(spec) == {"wl", "R"}):
        raise Exception("instruments: every instrument is {'newx': array}, {'R': r} (bins) or {'wl': array, 'R': r} "
                        "(a Gaussian line-spread function)")
    return tuple((k, np.shape(spec[k]), np.ascontiguousarray(spec[k], dtype=float).tobytes()) for k in sorted(spec))


def instruments_plan(opacityclass_or_wno, instruments, scale=1.0):
    """The ``InstrumentsPlan`` of a wavenumber grid (an opacity object, or the array itself) for ``instruments``:
    ``{name: {'newx': x}}`` (bins around ``x``, ``mean_regrid``'s; ``{'R': r}`` likewise) or ``{name: {'wl': wl, 'R': R}}``
    (``conv_non_uniform_R``'s Gaussian at the wavelengths ``wl``), in the order the output is wanted.  With an opacity
    object the plan is kept on it by content, as its members are: equal names and values give the same plan again."""
    from . import convolve as _convolve
    if not isinstance(instruments, dict) or not instruments:
        raise Exception("instruments must be a non-empty dictionary {name: {'newx': x} | {'wl': wl, 'R': R}}")
    wno = getattr(opacityclass_or_wno, "wno", None)

    def member(spec):
        if "wl" in spec:
            return _convolve.convolve_plan(opacityclass_or_wno, spec["wl"], spec["R"])
        return regrid_plan(opacityclass_or_wno, newx=spec.get("newx"), R=spec.get("R"))
    keys = tuple((name, _member_key(spec)) for name, spec in instruments.items())
    if wno is None:
        return InstrumentsPlan(opacityclass_or_wno, {n: member(s) for n, s in instruments.items()}, scale)
    cache = opacityclass_or_wno.__dict__.setdefault("_instrument_plans", {})
    hit = cache.get(keys)
    if hit is None or hit.wno is not wno:
        if len(cache) > 16:
            cache.clear()
        hit = cache[keys] = InstrumentsPlan(wno, {n: member(s) for n, s in instruments.items()}, 1.0)
    return hit.with_scale(scale)


def resolve_instruments(instruments, opa):
    """``instruments=`` of the public calls -> a plan on ``opa``'s grid: an ``InstrumentsPlan`` or the dictionary of
    ``instruments_plan``."""
    if isinstance(instruments, InstrumentsPlan):
        return instruments.check_grid(opa)
    return instruments_plan(opa, instruments)


def spectral_rows(albedo, thermal, transit, stellar, sa, radius_star, planet_radius):
    """The rows of one call in the order of the output dictionary -- ``[(key, op, a, b, c, k1, k2)]`` -- and the keys that
    stay list-valued placeholders, exactly where ``_post_reflected`` / ``_post_thermal`` / ``_post_final`` put them
    (justdoit.py:552-599).  ``albedo`` / ``thermal`` / ``transit`` / ``stellar``: device vectors (or None)."""
    rows, lists = [], {}
    k_r = k_t = None
    if albedo is not None:
        rows.append(("albedo", 0, albedo, None, None, 0.0, 0.0))
        if (not np.isnan(sa)) and (not np.isnan(planet_radius)):
            k_r = (planet_radius / sa) ** 2.0
            rows.append(("fpfs_reflected", 1, albedo, None, None, k_r, 0.0))
        else:
            lists["fpfs_reflected"] = []
    if thermal is not None:
        rows.append(("thermal", 0, thermal, None, None, 0.0, 0.0))
        if radius_star == "nostar":
            lists["fpfs_thermal"] = ["No star mode for Brown Dwarfs was used"]
        elif (not np.isnan(planet_radius)) and (not np.isnan(radius_star)):
            k_t = (planet_radius / radius_star) ** 2.0
            rows.append(("fpfs_thermal", 2, thermal, stellar, None, k_t, 0.0))
        else:
            lists["fpfs_thermal"] = []
    if transit is not None:
        rows.append(("transit_depth", 0, transit, None, None, 0.0, 0.0))
    if k_r is not None and k_t is not None:
        rows.append(("fpfs_total", 3, thermal, stellar, albedo, k_t, k_r))
    return rows, lists


class Binned:
    """The reduction of one call, enqueued: ``wait()`` -> ``({key: (nout) array}, [tail scalars])``."""

    def __init__(self, plan, ctx, rows, tails=(), keep=None):
        """``rows``: ``spectral_rows``'s.  ``tails``: device addresses of single doubles (the spectrum-wide integrals behind
        the result vectors) that travel in the same copy.  Everything is enqueued on ``ctx``'s stream: the caller has
        ordered it behind the producers of the inputs."""
        if not 1 <= len(rows) <= MAX_ROWS:
            raise Exception("%s: %d rows (1 to %d)" % (plan.kind, len(rows), MAX_ROWS))
        lib = _lib.load()
        nb, nr = plan.nout, len(rows)
        self.plan, self.keys, self.ntail = plan, [r[0] for r in rows], len(tails)
        crow = (_Row * nr)()
        for w, (_, op, a, b, c, k1, k2) in zip(crow, rows):
            w.op, w.a, w.b, w.c, w.k1, w.k2 = op, _lib.addr(a), _lib.addr(b), _lib.addr(c), float(k1), float(k2)
        self.out = DeviceArray((nr * nb + len(tails),), ctx)
        d_start = plan.launch(ctx, nr, crow, self.out.addr)
        for i, t in enumerate(tails):
            _lib.check(lib.picaso_memcpy_d2d(ctx, self.out.addr + 8 * (nr * nb + i), _lib.addr(t), 8), ctx)
        self.pin = self.out.to_host_async(device.PinnedArray(self.out.shape, ctx), ctx)
        self.keep = (keep, rows, d_start)          # the launch is asynchronous: its inputs live until the copy has landed

    def wait(self):
        a = self.pin.wait()
        nb = self.plan.nout
        vals = {k: a[i * nb:(i + 1) * nb].copy() for i, k in enumerate(self.keys)}
        tails = [a[len(self.keys) * nb + i] for i in range(self.ntail)]
        self.pin.free()
        self.pin = self.out = self.keep = None
        return vals, tails

    def abandon(self):
        if self.pin is not None:
            self.pin.free()
            self.pin = self.out = self.keep = None


def output(plan, vals, lists, bond_albedo=None, effective_temperature=None):
    """The output dictionary of a binned or convolved call: the keys of the plain one in its order, the plan's counts
    (``regrid_counts`` / ``convolve_counts``) added."""
    out = {"wavenumber": plan.out_wavenumber}

    def put(key):
        if key in vals:
            out[key] = vals[key]
        elif key in lists:
            out[key] = lists[key]
    if "albedo" in vals:
        put("albedo")
        out["bond_albedo"] = bond_albedo
        put("fpfs_reflected")
    if "thermal" in vals:
        put("thermal")
        out["thermal_unit"] = "erg/s/(cm^2)/(cm)"
        out["effective_temperature"] = effective_temperature
        put("fpfs_thermal")
    put("transit_depth")
    put("fpfs_total")
    out[plan.counts_key] = plan.counts
    return out
