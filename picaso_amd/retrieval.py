"""Posterior prediction bands on the device: ``get_evaluations`` and ``get_chisq_max`` (reference retrieval.py:199-367).

A retrieval ends by drawing ``n_draws`` samples from the equally weighted posterior, evaluating the model at each and
reducing the stack of spectra to the median and the 1, 2 and 3 sigma bands per wavelength (and the stack of profiles per
pressure level).  The reference reduces through ``ultranest.plot.PredictionBand``, whose ``get_line(q)`` is
``scipy.stats.mstats.mquantiles(ys, q, axis=0)[0]``: one host sort of every column per line, seven lines per stack.

Here a line is a row ``(k, gamma)`` of mquantiles' table, built on the host with scipy's own expressions
(``quantile_table``), and ``picaso_column_quantiles_dev`` (csrc/quantile.hip) sorts every column once in LDS and reads all
lines off it: ``(1. - gamma) * x[k - 1] + gamma * x[k]`` with numpy's rounding, so a band equals mquantiles' by value, bit
for bit.  Neither scipy nor ultranest is needed.
"""
import numpy as np

from . import _lib
from ._lib import PicasoHipError
from .analyze import chi_squared
from .device import DeviceArray
from .justdoit import mean_regrid

MAX_DRAWS = 16384       # PICASO_BANDS_MAX_DRAWS
MAX_Q = 32              # PICASO_BANDS_MAX_Q

# the reference's seven levels in its own expressions (retrieval.py:288-296)
SIGMA_QUANTILES = {}
for _k, _key in zip([k / 100 / 2 for k in [68.27, 95.45, 99.73]], ['1sig', '2sig', '3sig']):
    SIGMA_QUANTILES[_key + '_lo'] = 0.5 - _k
    SIGMA_QUANTILES[_key + '_hi'] = 0.5 + _k
SIGMA_QUANTILES['median'] = 0.5
del _k, _key


def quantile_table(n, q, alphap=0.4, betap=0.4):
    """``(k int32, gamma float64)`` of the levels ``q`` for ``n`` draws: the table of scipy's ``_quantiles1D``
    (scipy/stats/_mstats_basic.py), operation for operation.  A line is ``(1. - gamma) * x[k - 1] + gamma * x[k]`` on the
    sorted column ``x``.  ``n == 1`` has no table (the line is ``x[0]``): ``k = 1``, ``gamma = 0`` stand in."""
    p = np.atleast_1d(np.asarray(q, dtype=float))
    if p.ndim != 1:
        raise Exception("quantile_table: q must be a scalar or a 1-D sequence of levels")
    if np.any(np.isnan(p)) or np.any(p < 0) or np.any(p > 1):
        raise Exception("quantile_table: every level must lie in [0, 1]")
    n = int(n)
    if n < 1:
        raise Exception("quantile_table: n must be positive, got %d" % n)
    if n == 1:
        return np.ones(p.size, dtype=np.int32), np.zeros(p.size)
    m = alphap + p * (1. - alphap - betap)
    aleph = (n * p + m)
    k = np.floor(aleph.clip(1, n - 1)).astype(int)
    gamma = (aleph - k).clip(0, 1)
    return k.astype(np.int32), gamma


def _levels(q):
    """The levels of ``q``: a scalar, a sequence, or a dictionary like ``SIGMA_QUANTILES`` (its values, in its order)."""
    if isinstance(q, dict):
        q = list(q.values())
    return np.atleast_1d(np.asarray(q, dtype=float))


def column_quantiles(d_y, k, gamma, cols=None):
    """``picaso_column_quantiles_dev`` on the resident ``(S, N)`` DeviceArray ``d_y``: the ``(nq, ncol)`` DeviceArray of
    the lines ``(k, gamma)`` of its columns, or of the columns ``cols = (lo, hi)`` alone (the matrix's row stride stays
    ``N``).  The launch is asynchronous; the result keeps its input alive."""
    if len(d_y.shape) != 2:
        raise PicasoHipError("column_quantiles: the matrix must be (S, N), got %s" % (d_y.shape,))
    S, N = d_y.shape
    lo, hi = (0, N) if cols is None else (int(cols[0]), int(cols[1]))
    if not 0 <= lo < hi <= N:
        raise PicasoHipError("column_quantiles: columns [%d, %d) lie outside the matrix's %d" % (lo, hi, N))
    k = np.ascontiguousarray(k, dtype=np.int32)
    gamma = np.ascontiguousarray(gamma, dtype=np.float64)
    if k.ndim != 1 or gamma.shape != k.shape:
        raise PicasoHipError("column_quantiles: k and gamma must be 1-D and of one length, got %s and %s"
                             % (k.shape, gamma.shape))
    if not 1 <= k.size <= MAX_Q:
        raise PicasoHipError("column_quantiles: %d levels; one call takes 1 to %d" % (k.size, MAX_Q))
    ctx = d_y.ctx
    out = DeviceArray((k.size, hi - lo), ctx)
    _lib.check(_lib.load().picaso_column_quantiles_dev(ctx, S, hi - lo, d_y.addr + 8 * lo, N, k.size, k.ctypes.data,
                                                       gamma.ctypes.data, out.addr), ctx)
    out._inputs = (d_y,)
    return out


def _reduce(ys, k, gamma):
    """The lines ``(k, gamma)`` of the columns of ``ys`` -- a host ``(S, N)`` array (one upload) or a DeviceArray -- as a
    host ``(nq, N)`` array: one launch, one copy back."""
    if not isinstance(ys, DeviceArray):
        ys = DeviceArray.from_host(ys)
    return column_quantiles(ys, k, gamma).to_host()


def _matrix_shape(ys):
    shape = tuple(ys.shape) if isinstance(ys, DeviceArray) else np.shape(ys)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise Exception("bands: ys must be a non-empty (S, N) matrix, one row per draw; got shape %s" % (shape,))
    if shape[0] > MAX_DRAWS:
        raise Exception("bands: %d draws; a column is sorted in LDS and takes at most %d" % (shape[0], MAX_DRAWS))
    return shape


@_lib.serialized
def bands(ys, q=SIGMA_QUANTILES):
    """``mquantiles(ys, q, axis=0)`` of the ``(S, N)`` stack ``ys`` (one row per draw): ``(len(q), N)``, row ``i`` what
    ``PredictionBand.get_line(q[i])`` returns.  ``ys``: a host array (uploaded once) or a ``DeviceArray``; ``q``: levels,
    or a dictionary of them (its values, in its order; the default: the reference's seven lines).  One launch, and
    only the result is copied back.  At most 16 384 draws and 32 levels per call."""
    S, _ = _matrix_shape(ys)
    p = _levels(q)
    if not 1 <= p.size <= MAX_Q:
        raise Exception("bands: %d levels; one call takes 1 to %d" % (p.size, MAX_Q))
    k, gamma = quantile_table(S, p)
    if not isinstance(ys, DeviceArray):
        ys = np.ascontiguousarray(ys, dtype=np.float64)
    return _reduce(ys, k, gamma)


class PredictionBand(object):
    """Stand-in for ``ultranest.plot.PredictionBand``: collect the model ``y(x)`` of every draw with ``add``, read the
    quantile lines with ``get_line``.  The rows are kept on the host; the first ``get_line`` after an ``add`` uploads the
    matrix, and every further one reuses that copy."""

    def __init__(self, x):
        self.x = x
        self.ys = []
        self._dev = None

    def add(self, y):
        y = np.asarray(y, dtype=float)
        if y.shape != np.shape(self.x):
            raise Exception("PredictionBand.add: y has shape %s, x has %s" % (y.shape, np.shape(self.x)))
        self.ys.append(y)
        self._dev = None

    def _matrix(self):
        if not self.ys:
            raise Exception("PredictionBand: no rows have been added")
        if self._dev is None:
            if len(self.ys) > MAX_DRAWS:
                raise Exception("PredictionBand: %d rows; the bands take at most %d" % (len(self.ys), MAX_DRAWS))
            self._dev = DeviceArray.from_host(np.array(self.ys))
        return self._dev

    @_lib.serialized
    def lines(self, q):
        """``(len(q), len(x))``: the lines of all levels ``q`` from one launch."""
        return bands(self._matrix(), q)

    def get_line(self, q=0.5):
        return self.lines([q])[0]


def _profile(picaso_class):
    """The profile behind ``model(..., return_ptchem=True)``: the inputs object's, or that of the first entry when the
    model returns a dictionary of them (reference retrieval.py:239-244)."""
    if isinstance(picaso_class, dict):
        picaso_class = picaso_class[list(picaso_class.keys())[0]]
    return picaso_class.inputs['atmosphere']['profile']


def get_evaluations(samples_equal, max_logl, model, n_draws, regrid=False, pressure_bands=['temperature', 'H2O', 'CO2']):
    """The model at the best sample and the 1, 2 and 3 sigma bands of spectra, temperature and abundances (reference
    retrieval.py:199-310).

    ``samples_equal`` (nsamples, nparams): the equally weighted posterior; ``max_logl``: the parameters of the best
    sample; ``model(params)`` returns ``(wavenumber, spectrum, offsets, error_inflation)`` and ``model(params,
    return_ptchem=True)`` the inputs object (or a one-entry dictionary of them) whose ``inputs['atmosphere']['profile']``
    -- a DataFrame or a dictionary of columns -- holds ``pressure`` and every name of ``pressure_bands``
    (``pressure_bands=[]`` for a model without one).  ``n_draws`` rows are drawn with ``np.random.randint(0,
    samples_equal.shape[0], n_draws)``: after ``np.random.seed`` they are the reference's draws.  ``regrid``: a
    wavenumber array or a float resolution, applied to every draw through ``mean_regrid``; ``False``: spectra as the model
    returns them.

    Returns the reference's dictionary: ``max_logl_ptchem``, ``bands_spectra`` (``1sig_lo`` ... ``3sig_hi``, ``median``),
    ``bands_ptchem`` (the same per name of ``pressure_bands``), ``max_logl_spectra``, ``max_logl_error_inflation``,
    ``max_logl_offsets``, ``pressure``, ``wavelength``.  The spectra of all draws are reduced in one launch, the
    profiles of all names in a second one.

    One deviation: with ``regrid=False`` the reference never sets ``binning`` and raises ``NameError`` at its last step;
    here ``max_logl_spectra`` is then the unbinned spectrum of the best sample."""
    if n_draws < 1:
        raise Exception("get_evaluations: n_draws must be positive")
    if n_draws > MAX_DRAWS:
        raise Exception("get_evaluations: %d draws; the bands take at most %d" % (n_draws, MAX_DRAWS))
    returns = {}
    names = list(pressure_bands)
    if len(names) > 0:
        returns['max_logl_ptchem'] = _profile(model(max_logl, return_ptchem=True))
        df = returns['max_logl_ptchem']

    draws = np.random.randint(0, samples_equal.shape[0], n_draws)

    binning = False
    spectra, profiles = [], []
    for idraw in draws:
        x, y, of, er = model(samples_equal[idraw, :])
        if len(names) > 0:
            chem = _profile(model(samples_equal[idraw, :], return_ptchem=True))
            profiles.append(np.concatenate([np.asarray(chem[i], dtype=float) for i in names]))
        if isinstance(regrid, np.ndarray):          # assumed to be a wavenumber grid
            _, y = mean_regrid(x, y, newx=regrid)
            binning = True
            um_xgrid = 1e4 / regrid
        elif isinstance(regrid, float):
            wno_xgrid, y = mean_regrid(x, y, R=regrid)
            binning = True
            um_xgrid = 1e4 / wno_xgrid
        else:
            um_xgrid = 1e4 / x
        spectra.append(np.asarray(y, dtype=float))

    keys = list(SIGMA_QUANTILES.keys())
    k, gamma = quantile_table(n_draws, _levels(SIGMA_QUANTILES))
    lines = _reduce(np.array(spectra), k, gamma)
    returns['bands_spectra'] = {key: lines[i] for i, key in enumerate(keys)}
    if len(names) > 0:
        nlevel = np.asarray(df['pressure']).size
        lines = _reduce(np.array(profiles), k, gamma)
        returns['bands_ptchem'] = {name: {key: lines[i, j * nlevel:(j + 1) * nlevel] for i, key in enumerate(keys)}
                                   for j, name in enumerate(names)}

    maxx, maxlogl, offsets, err = model(max_logl)
    if binning:
        _, maxlogl = mean_regrid(maxx, maxlogl, newx=1e4 / um_xgrid)
    returns['max_logl_spectra'] = maxlogl
    returns['max_logl_error_inflation'] = err
    returns['max_logl_offsets'] = offsets
    if len(names) > 0:
        returns['pressure'] = df['pressure']
    returns['wavelength'] = um_xgrid
    return returns


def get_chisq_max(at_evaluations, data_dict):
    """Chi squared per data point of the best sample's spectrum (reference retrieval.py:312-367), on the host.
    ``at_evaluations``: ``get_evaluations``' dictionary; ``data_dict``: ``{name: (wavenumber, y, e)}``.  The spectrum is
    binned to every data set with ``mean_regrid``, the data get the set's offset (``max_logl_offsets``, 0 without one),
    everything is ordered by wavenumber.  Returns ``wavenumber``, ``model``, ``datay``, ``datae`` and
    ``chisq_per_datapt``."""
    offsets = at_evaluations['max_logl_offsets']
    resultx, resulty = 1e4 / at_evaluations['wavelength'], at_evaluations['max_logl_spectra']
    y_model_all, x_data_all, y_data_all, e_data_all = [], [], [], []
    for idata in data_dict.keys():
        if idata in offsets.keys():
            offset = offsets[idata]
        else:
            offset = 0
        x_chunk, y_chunk = mean_regrid(resultx, resulty, newx=data_dict[idata][0])
        y_model_all += [y_chunk]
        x_data_all += [x_chunk]
        y_data_all += [data_dict[idata][1] + offset]
        e_data_all += [data_dict[idata][2]]
    x = np.concatenate(x_data_all)
    order = np.argsort(x, kind='quicksort')            # DataFrame.sort_values' default
    sorted_x = x[order]
    sorted_y = np.concatenate(y_model_all)[order]
    datasorted_y = np.concatenate(y_data_all)[order]
    datasorted_e = np.concatenate(e_data_all)[order]
    chisq = chi_squared(datasorted_y, datasorted_e, sorted_y, 0)
    return {'wavenumber': sorted_x, 'model': sorted_y, 'datay': datasorted_y, 'datae': datasorted_e,
            'chisq_per_datapt': chisq}
