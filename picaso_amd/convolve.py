"""Spectra convolved with an instrument's line-spread function on the device: ``spectrum(convolve=...)``.

Data whose resolving power changes along the spectrum (a prism) is compared with a model that has been convolved with a
Gaussian of ``sigma_i = wl_i / R_i / 2.355`` and evaluated at every observed wavelength ``wl_i``: the reference's retrieval
driver carries it as ``conv_non_uniform_R`` (driver.py:338-381), ``nobs x nwno`` evaluations of ``exp`` per spectral array
on the host, behind the copies of the full-resolution arrays.  Here the window of every point is found once per grid
(``ConvolvePlan``), the weighted sums are formed on the device behind the solvers together with the flux ratios of the
output dictionary (``picaso_lsf_convolve_dev``, csrc/convolve.hip: the weight of a column is computed once and shared by
all arrays of the call), and ``nobs`` doubles per output come back.  It plugs into the seam ``regrid=`` made
(``regrid.Reduction``): same rows, same single copy, same scope.

A window is every column within 39 sigma of the point.  Beyond it the reference's weight is ``exp(-760.5)`` and less, an
exact ``0.0`` in fp64 (the smallest subnormal is ``exp(-744.4)``), which adds nothing to either of its sums: the windowed
sums run over exactly the reference's non-zero terms.  The argument of ``exp`` has numpy's bits on the device, so a
convolved array differs from ``conv_non_uniform_R`` of the plain call's array by the rounding of ``exp`` and the order of two
sums of ``counts[i]`` non-negative weights: at most ``(2 counts[i] + 10) 2^-53`` of ``conv(|array|)``.
"""
import weakref

import numpy as np

from . import _lib
from . import regrid as _regrid
from .device import DeviceArray

NSIGMA = 39.0            # |d| > 39 sigma: d^2 / (2 sigma^2) > 760.5, exp(-760.5) == 0.0
_plans = weakref.WeakSet()


def _resolution(R, wl):
    """``R`` per observed point as float64: a scalar, or one value per point."""
    R = np.asarray(R, dtype=float)
    if R.ndim == 0:
        R = np.full(wl.shape, float(R))
    if R.shape != wl.shape:
        raise Exception("convolve: R and wl have different lengths (%s and %s): R is a scalar or one value per point"
                        % (R.shape, wl.shape))
    if not np.all(R > 0):                       # NaN included
        raise Exception("convolve: R must be positive")
    return R


def _sigma_den(wl, R):
    """``sigma`` and ``2 sigma^2`` per point, formed point by point on numpy scalars as the reference forms them (its
    ``sigma ** 2`` is the C library's ``pow``, which an array's square need not equal in the last bit)."""
    sigma = np.array([w / r / 2.355 for w, r in zip(wl, R)], dtype=float).reshape(wl.shape)
    den = np.array([2 * s ** 2 for s in sigma], dtype=float).reshape(wl.shape)
    return sigma, den


def conv_non_uniform_R(model_flux, model_wl, R, obs_wl):
    """The model spectrum ``model_flux`` on ``model_wl`` seen at every ``obs_wl[i]`` through a Gaussian line-spread
    function of resolving power ``R[i]`` (FWHM ``obs_wl[i] / R[i]``), normalised over the model grid: the reference's
    function of this name (driver.py:338-381), in numpy on the host, ``len(obs_wl) x len(model_wl)`` weights.  ``R``: one
    value per observed point (a scalar is taken for all of them).  A point without any weight on the model grid is NaN."""
    model_flux, model_wl = np.asarray(model_flux), np.asarray(model_wl)
    obs_wl = np.asarray(obs_wl)
    R = np.broadcast_to(np.asarray(R), obs_wl.shape)
    out = np.zeros_like(obs_wl)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i, centre in enumerate(obs_wl):
            sigma = centre / R[i] / 2.355
            weight = np.exp(-((model_wl - centre) ** 2) / (2 * sigma ** 2))
            weight /= np.sum(weight)
            out[i] = np.sum(model_flux * weight)
    return out


class ConvolvePlan(_regrid.Reduction):
    """The windows of ``nobs`` observed points on one wavenumber grid: ``wl`` (um, the caller's order), ``R`` (per point),
    ``model_wl = 1e4 / wno``, ``centre`` (= ``wl``), ``den = 2 sigma^2``, and per point the contiguous column range
    ``[lo[i], hi[i])`` of the model wavelengths within 39 sigma, ``counts = hi - lo``.  The tables are uploaded once per
    context, when a spectrum first uses the plan."""
    kind, counts_key = "convolve", "convolve_counts"
    nout = property(lambda self: self.nobs)

    def __init__(self, wno, wl, R):
        x = np.asarray(wno, dtype=float)
        if x.ndim != 1 or x.size < 1:
            raise Exception("convolve_plan: the wavenumber grid must be a non-empty 1-D array")
        step = np.diff(x)
        if not (np.all(step > 0) or np.all(step < 0)) or not np.all(x > 0):
            raise Exception("convolve_plan: the wavenumber grid must be positive and strictly monotone")
        wl = np.array(wl, dtype=float)
        if wl.ndim != 1 or wl.size < 1:
            raise Exception("convolve_plan: wl must be a non-empty 1-D array of wavelengths (um)")
        if not (np.all(np.isfinite(wl)) and np.all(wl > 0)):
            raise Exception("convolve_plan: the wavelengths must be positive and finite")
        R = _resolution(R, wl)
        sigma, den = _sigma_den(wl, R)
        model_wl = 1e4 / x
        n = x.size
        if n > 1 and model_wl[0] > model_wl[-1]:            # the usual case: wavenumbers increase, wavelengths decrease
            asc = model_wl[::-1]
            hi = n - np.searchsorted(asc, wl - NSIGMA * sigma, side="left")
            lo = n - np.searchsorted(asc, wl + NSIGMA * sigma, side="right")
        else:
            lo = np.searchsorted(model_wl, wl - NSIGMA * sigma, side="left")
            hi = np.searchsorted(model_wl, wl + NSIGMA * sigma, side="right")
        hi = np.maximum(hi, lo)
        self.wno, self.nwno, self.nobs = wno, int(n), int(wl.size)
        self.wl, self.R, self.sigma = wl, R, sigma
        self.model_wl, self.centre, self.den = model_wl, wl, den
        self.out_wavenumber = 1e4 / wl
        self.lo, self.hi = lo.astype(np.int32), hi.astype(np.int32)
        self.counts = (hi - lo).astype(np.int64)
        for a in (self.wl, self.R, self.sigma, self.model_wl, self.den, self.out_wavenumber, self.lo, self.hi, self.counts):
            a.flags.writeable = False
        self._dev = {}
        _plans.add(self)

    def device_tables(self, ctx):
        """``(model_wl, centre, den, windows)`` in HBM on ``ctx``'s device; ``windows`` holds ``lo`` then ``hi`` as int32
        (carried by a float64 DeviceArray of the same bytes)."""
        key = getattr(ctx, "value", ctx)
        hit = self._dev.get(key)
        if hit is None:
            win = np.zeros((2 * self.nobs + 1) // 2 * 2, dtype=np.int32)
            win[:self.nobs], win[self.nobs:2 * self.nobs] = self.lo, self.hi
            hit = self._dev[key] = tuple(DeviceArray.from_host(a, ctx) for a in
                                         (self.model_wl, self.centre, self.den, win.view(np.float64)))
        return hit

    def launch(self, ctx, nrows, crows, out_addr):
        tables = d_wl, d_c, d_den, d_win = self.device_tables(ctx)
        _lib.check(_lib.load().picaso_lsf_convolve_dev(
            ctx, self.nwno, d_wl.addr, self.nobs, d_c.addr, d_den.addr, d_win.addr, d_win.addr + 4 * self.nobs,
            nrows, crows, out_addr), ctx)
        return tables


def _drop_context(value):
    """``destroy_context``: a new context may be created at the same address later."""
    for plan in list(_plans):
        plan._dev.pop(value, None)


_lib.on_context_destroy(_drop_context)


def convolve_plan(opacityclass_or_wno, wl, R):
    """The ``ConvolvePlan`` of a wavenumber grid (an opacity object, or the array itself) for data at the wavelengths
    ``wl`` (um; any order, duplicates allowed) of resolving power ``R`` (a scalar, or one value per point).  With an opacity
    object the plan is kept on it by content: equal ``wl`` and ``R`` values give the same plan again, and its tables are
    uploaded once."""
    wno = getattr(opacityclass_or_wno, "wno", None)
    if wno is None:
        return ConvolvePlan(opacityclass_or_wno, wl, R)
    opa = opacityclass_or_wno
    a = np.ascontiguousarray(wl, dtype=float)
    r = np.ascontiguousarray(R, dtype=float)
    key = (a.shape, a.tobytes(), r.shape, r.tobytes())
    cache = opa.__dict__.setdefault("_convolve_plans", {})
    hit = cache.get(key)
    if hit is None or hit.wno is not wno:
        if len(cache) > 16:
            cache.clear()
        hit = cache[key] = ConvolvePlan(wno, wl, R)
    return hit


def resolve(convolve, opa):
    """``convolve=`` of the public calls -> a plan on ``opa``'s grid: a ``ConvolvePlan`` or ``{'wl': array, 'R': r}``."""
    if isinstance(convolve, ConvolvePlan):
        return convolve.check_grid(opa)
    if isinstance(convolve, dict) and set(convolve) == {"wl", "R"}:
        return convolve_plan(opa, convolve["wl"], convolve["R"])
    raise Exception("convolve must be a convolve_plan() or {'wl': array, 'R': scalar_or_array}")


def reduction(regrid, convolve, opa, instruments=None):
    """The plan of a public call from its three keywords (None: a plain call); more than one at once is an error."""
    given = sum(k is not None for k in (regrid, convolve, instruments))
    if given > 1 and instruments is None:
        raise Exception("regrid= and convolve= are two ways from the model grid to the data's: give one of them")
    if given > 1:
        raise Exception("regrid=, convolve= and instruments= are three ways from the model grid to the data's: give one "
                        "of them (instruments= takes a binned and a convolved data set together)")
    if regrid is not None:
        return _regrid.resolve(regrid, opa)
    if convolve is not None:
        return resolve(convolve, opa)
    if instruments is not None:
        return _regrid.resolve_instruments(instruments, opa)
    return None
