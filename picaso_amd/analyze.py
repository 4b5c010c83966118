"""Model grids fitted to data on the device: ``GridFitter`` and ``custom_interp`` (reference analyze.py).

The reference ranks the models of a grid against a data set in a Python loop -- ``mean_regrid`` per model, a
``curve_fit`` for a constant offset, ``chi_squared`` (analyze.py:305-388) -- and samples between the grid nodes with a
recursive gather of the ``2^d`` corner spectra per likelihood evaluation (``custom_interp``, analyze.py:923-1000).  Here the
grid's spectra are uploaded once; every sample -- a model of the grid, or a point between its nodes -- is a short table of
(row, weight) pairs and a divisor, ``picaso_grid_rows_dev`` (csrc/gridfit.hip) forms the weighted sums for all samples in
one launch, either in full or already binned to the data's grid, and ``picaso_grid_loglike_dev`` reduces the binned
models against the data, one workgroup per sample.

The tables are built on the host with the reference's own expressions in vectorised numpy, and the kernel takes the
products and additions in table order with numpy's rounding, so an interpolated spectrum has ``custom_interp``'s bits,
and its binned form those of ``mean_regrid`` of it.  Only the sums over the data points (the offset, chi squared, the log
likelihood) run in another order than numpy's pairwise one; they differ from the reference by rounding.

``bands_batch`` ends a gridtrieval: the quantile lines (median, 1, 2 and 3 sigma) over the spectra interpolated to the
posterior's draws, read off the resident result by ``picaso_column_quantiles_dev`` (``picaso_amd/retrieval.py``).
"""
import itertools

import numpy as np

from . import _lib
from ._lib import PicasoHipError
from .device import DeviceArray
from .regrid import RegridPlan

MAX_K = 64              # PICASO_GRID_MAX_K: 2^6 corners
MAX_DIM = 6


# ---------------------------------------------------------------------------------------------- host functions
def chi_squared(data, data_err, model, numparams):
    """Reduced chi squared with ``len(data) - numparams`` degrees of freedom (reference analyze.py:1315-1333)."""
    return np.sum(((data - model) / (data_err)) ** 2) / (len(data) - (numparams))


def get_last_dimension(arr, indices):
    """``arr[i0, i1, ..., :]`` for ``indices = [i0, i1, ..., -1]``: the last entry, -1, stands for ``:`` (reference
    analyze.py:1002-1028)."""
    if len(indices) == 1 and indices[0] == -1:
        return arr
    elif len(indices) == 1:
        return arr[indices[0]]
    return get_last_dimension(arr[indices[0]], indices[1:])


def find_bounding_values(arr, value):
    """The two nodes of the sorted ``arr`` around ``value`` and their indices, ``([lower, upper], [i, i + 1])``; at or
    above the last node: the last two nodes; below the first: ``[arr[0]]`` alone (reference analyze.py:1030-1063)."""
    indices = np.where(arr <= value)[0]
    if len(indices) == 0:
        return [arr[0]]
    if indices[-1] == len(arr) - 1:
        return [arr[-2], arr[-1]], [indices[-1] - 1, indices[-1]]
    return [arr[indices[-1]], arr[indices[-1] + 1]], [indices[-1], indices[-1] + 1]


def _finditem(obj, key):
    if key in obj:
        return obj[key]
    for k, v in obj.items():
        if isinstance(v, dict):
            item = _finditem(v, key)
            if item is not None:
                return item


# ---------------------------------------------------------------------------------------------- device plumbing
def _upload_i32(a, ctx):
    """int32 values in HBM, carried by a float64 DeviceArray of the same bytes (as ``RegridPlan.device_start``)."""
    a = np.ascontiguousarray(a, dtype=np.int32).ravel()
    padded = np.zeros((a.size + 1) // 2 * 2, dtype=np.int32)
    padded[:a.size] = a
    return DeviceArray.from_host(padded.view(np.float64), ctx)


def grid_rows(ctx, d_grid, nrows, nwave, rows, wts, kcount, div, plan=None, full=False):
    """``picaso_grid_rows_dev`` for host tables ``rows`` / ``wts`` ``(S, K)``, ``kcount`` / ``div`` ``(S)`` on the resident
    matrix ``d_grid`` ``(nrows, nwave)``: the ``(S, nwave)`` DeviceArray of the weighted sums (``full``) or the
    ``(S, plan.nbins)`` one of their bin means (``plan``: a ``RegridPlan`` on the matrix's columns).  The tables are
    checked here, before anything is uploaded: a row index outside ``[0, nrows)`` or a count outside ``[1, K]`` is a
    ``PicasoHipError`` and nothing is launched."""
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    wts = np.ascontiguousarray(wts, dtype=np.float64)
    kcount = np.ascontiguousarray(kcount, dtype=np.int32)
    div = np.ascontiguousarray(div, dtype=np.float64)
    if rows.ndim != 2 or wts.shape != rows.shape or kcount.shape != rows.shape[:1] or div.shape != rows.shape[:1]:
        raise PicasoHipError("grid_rows: rows and wts must be (S, K), kcount and div (S); got %s, %s, %s, %s"
                             % (rows.shape, wts.shape, kcount.shape, div.shape))
    S, K = rows.shape
    if not 1 <= K <= MAX_K:
        raise PicasoHipError("grid_rows: K must be in [1, %d], got %d" % (MAX_K, K))
    if S < 1:
        raise PicasoHipError("grid_rows: no samples")
    if np.any(kcount < 1) or np.any(kcount > K):
        raise PicasoHipError("grid_rows: a sample's count is outside [1, %d] (%d to %d)" % (K, kcount.min(), kcount.max()))
    used = np.arange(K)[None, :] < kcount[:, None]
    bad = used & ((rows < 0) | (rows >= nrows))
    if np.any(bad):
        s, c = np.argwhere(bad)[0]
        raise PicasoHipError("grid_rows: sample %d, entry %d: row index %d outside [0, %d)" % (s, c, rows[s, c], nrows))
    if (plan is None) == (not full):
        raise PicasoHipError("grid_rows: ask for the full form or give a plan for the binned one")
    if plan is not None and plan.nwno != nwave:
        raise PicasoHipError("grid_rows: the plan was made for %d columns, the matrix has %d" % (plan.nwno, nwave))
    d_rows, d_wts = _upload_i32(rows, ctx), DeviceArray.from_host(wts, ctx)
    d_k, d_div = _upload_i32(kcount, ctx), DeviceArray.from_host(div, ctx)
    if full:
        out = DeviceArray((S, nwave), ctx)
        args = (out.addr, 0, None, None)
        d_start = None
    else:
        d_start = plan.device_start(ctx)
        out = DeviceArray((S, plan.nbins), ctx)
        args = (None, plan.nbins, d_start.addr, out.addr)
    _lib.check(_lib.load().picaso_grid_rows_dev(ctx, int(nrows), int(nwave), d_grid.addr, S, K, d_rows.addr, d_wts.addr,
                                                d_k.addr, d_div.addr, *args), ctx)
    out._inputs = (d_grid, d_rows, d_wts, d_k, d_div, d_start)      # the launch is asynchronous
    return out


def grid_loglike(ctx, d_binned, S, y, e, offset, scaling, err_inf):
    """``picaso_grid_loglike_dev`` mode 0: the ``(S)`` log likelihoods of the binned models ``d_binned`` ``(S, ndata)``."""
    y, e = _lib.f64(y), _lib.f64(e)
    n = y.size
    if e.shape != y.shape or y.ndim != 1 or tuple(d_binned.shape) != (S, n):
        raise Exception("y_data and e_data must be 1-D arrays of the data grid's length (%d), got %s and %s"
                        % (d_binned.shape[-1], y.shape, e.shape))
    per = [DeviceArray.from_host(_lib.f64(np.zeros(S) + np.asarray(v, dtype=float), (S,)), ctx)
           for v in (offset, scaling, err_inf)]
    d_y, d_e, out = DeviceArray.from_host(y, ctx), DeviceArray.from_host(e, ctx), DeviceArray((S,), ctx)
    _lib.check(_lib.load().picaso_grid_loglike_dev(ctx, S, n, d_binned.addr, d_y.addr, d_e.addr, 0, per[0].addr,
                                                   per[1].addr, per[2].addr, out.addr, 0, 0, None, None, None), ctx)
    return out.to_host()


def grid_chi2(ctx, d_binned, S, y, e, fit_offset, numparams):
    """``picaso_grid_loglike_dev`` mode 1: ``(shift (S), chi2 (S), best (S, ndata))``."""
    y, e = _lib.f64(y), _lib.f64(e)
    n = y.size
    if e.shape != y.shape or y.ndim != 1 or tuple(d_binned.shape) != (S, n):
        raise Exception("y_data and e_data must be 1-D arrays of the data grid's length (%d), got %s and %s"
                        % (d_binned.shape[-1], y.shape, e.shape))
    d_y, d_e = DeviceArray.from_host(y, ctx), DeviceArray.from_host(e, ctx)
    shift, chi2, best = DeviceArray((S,), ctx), DeviceArray((S,), ctx), DeviceArray((S, n), ctx)
    _lib.check(_lib.load().picaso_grid_loglike_dev(ctx, S, n, d_binned.addr, d_y.addr, d_e.addr, 1, None, None, None,
                                                   None, int(bool(fit_offset)), int(numparams), shift.addr, chi2.addr,
                                                   best.addr), ctx)
    return shift.to_host(), chi2.to_host(), best.to_host()


# ---------------------------------------------------------------------------------------------- the fitter
class _InterpParams(dict):
    """``interp_params[grid_name]``: the reference's keys; ``square_spectra_grid`` is built when it is first read."""

    def __missing__(self, key):
        if key != "square_spectra_grid":
            raise KeyError(key)
        spectra, node_rows = self["_spectra"], self["node_rows"]
        sq = np.full(node_rows.shape + (spectra.shape[1],), np.nan)
        have = node_rows >= 0
        sq[have] = spectra[node_rows[have]]
        self[key] = sq
        return sq


class GridFitter():
    """The reference's grid fitter (analyze.py:30-920) for grids handed over as arrays.

    ``GridFitter(grid_name, wavelength=..., spectra=..., grid_params=...)`` adds a first grid (``add_grid``);
    ``GridFitter()`` starts empty.  Reading a directory of xarray files (``model_dir``) is not available here."""

    def __init__(self, grid_name=None, model_dir=None, verbose=True, **arrays):
        self.verbose = verbose
        self.grids = []
        self.list_of_files = {}
        self.grid_params = {}
        self.overview = {}
        self.wavelength = {}
        self.temperature = {}
        self.save_chem = False
        self.pressure = {}
        self.spectra = {}
        self.interp_params = {}
        self._dev = {}
        self._plans = {}
        if model_dir is not None:
            raise NotImplementedError("GridFitter: reading a directory of xarray files (model_dir) needs xarray; load the "
                                      "models yourself and hand them to add_grid(grid_name, wavelength, spectra, grid_params)")
        if arrays:
            if grid_name is None:
                raise Exception("GridFitter: a grid needs a grid_name")
            self.add_grid(grid_name, **arrays)

    def add_grid(self, grid_name, wavelength, spectra, grid_params, temperature=None, pressure=None, chemistry=None):
        """Add the grid ``grid_name``: ``wavelength`` (nwave), ``spectra`` (nmodels, nwave) and ``grid_params``
        ``{'planet_params': {'mh': (nmodels,), ...}, ...}`` (the reference's layout, load_grid_params).  The spectra are
        uploaded once, when a device path first reads them.

        ``wavelength`` must be strictly monotonic.  A decreasing grid and its spectra are reversed once at upload (the
        bins are contiguous column ranges of an increasing grid), so a bin's sum then runs in the opposite order to the
        reference's, which adds in the order of the array it is given: the binned values of such a grid differ from the
        reference's by rounding only.  ``self.wavelength`` / ``self.spectra`` keep the caller's order, and so do the
        interpolated spectra.

        ``spectra`` must be finite or NaN: ``inf`` is an ``Exception``; a row with any NaN counts as a missing model."""
        wl = np.asarray(wavelength, dtype=float)
        sp = np.asarray(spectra, dtype=float)
        if wl.ndim != 1 or wl.size < 2:
            raise Exception("add_grid: wavelength must be a 1-D array of at least two points")
        if sp.ndim != 2 or sp.shape[1] != wl.size or sp.shape[0] < 1:
            raise Exception("add_grid: spectra must be (nmodels, %d), got %s" % (wl.size, sp.shape))
        d = np.diff(wl)
        if not (np.all(d > 0) or np.all(d < 0)):
            raise Exception("add_grid: wavelength must be strictly monotonic")
        if np.any(np.isinf(sp)):
            raise Exception("add_grid: spectra holds inf (it must be finite, or NaN for a missing model)")
        nmodels = sp.shape[0]
        params, overview, cnt = {}, {}, 0
        for iattr, group in grid_params.items():
            params[iattr], overview[iattr] = {}, {}
            for ikey, vals in group.items():
                vals = np.asarray(vals)
                if vals.shape != (nmodels,):
                    raise Exception("add_grid: grid_params[%r][%r] must be (%d,), got %s" % (iattr, ikey, nmodels, vals.shape))
                params[iattr][ikey] = vals
                uni = np.unique(vals)
                if len(uni) == 1:
                    overview[iattr][ikey] = uni[0]
                else:
                    overview[iattr][ikey] = uni
                    cnt += 1
                    if self.verbose:
                        print(f'For {ikey} in {iattr} grid is: {uni}')
        overview['num_params'] = cnt
        if grid_name not in self.grids:
            self.grids += [grid_name]
        self.list_of_files[grid_name] = list(range(nmodels))
        self.grid_params[grid_name] = params
        self.overview[grid_name] = overview
        self.wavelength[grid_name] = wl
        self.spectra[grid_name] = sp
        self.temperature[grid_name] = temperature
        self.pressure[grid_name] = pressure
        if chemistry is not None:
            self.save_chem = True
            self.chemistry = getattr(self, 'chemistry', {})
            self.chemistry[grid_name] = chemistry
        self.interp_params.pop(grid_name, None)
        for key in [k for k in self._plans if k[0] == grid_name]:
            del self._plans[key]
        flip = bool(d[0] < 0)
        self._dev[grid_name] = {"flip": flip, "nrows": nmodels, "nwave": wl.size,
                                "x": np.ascontiguousarray(wl[::-1]) if flip else wl,
                                "missing": np.any(np.isnan(sp), axis=1)}

    def _device(self, grid_name):
        """The grid's device record; its spectra go to HBM once, when a device path first needs them (building the
        tables of an interpolation needs no device)."""
        dev = self._dev[grid_name]
        if "spectra" not in dev:
            sp = self.spectra[grid_name]
            dev["ctx"] = _lib.context()
            dev["spectra"] = DeviceArray.from_host(np.ascontiguousarray(sp[:, ::-1]) if dev["flip"] else sp, dev["ctx"])
        return dev

    def add_data(self, data_name, wlgrid_center, wlgrid_width, y_data, e_data):
        """Add a data set: bin centres and widths, the values and their errors (reference analyze.py:120-141)."""
        self.data = getattr(self, 'data', {data_name: []})
        self.data[data_name] = {'wlgrid_center': wlgrid_center,
                                'wlgrid_width': wlgrid_width,
                                'y_data': y_data,
                                'e_data': e_data}
        for key in [k for k in self._plans if k[1] == data_name]:
            del self._plans[key]

    def as_dict(self):
        return {'list_of_files': self.list_of_files,
                'spectra_w_offset': self.best_fits,
                'rank_order': self.rank,
                'grid_params': self.grid_params,
                'offsets': getattr(self, 'offsets', 0),
                'chi_sqs': self.chi_sqs,
                'posteriors': self.posteriors}

    def _plan(self, grid_name, data_name):
        """The bins of the data set on the grid's (increasing) wavelengths, kept per (grid, data)."""
        key = (grid_name, data_name)
        hit = self._plans.get(key)
        if hit is None:
            hit = self._plans[key] = RegridPlan(self._dev[grid_name]["x"], newx=self.data[data_name]['wlgrid_center'])
        return hit

    def fit_all(self):
        for i in self.grids:
            for j in self.data.keys():
                self.fit_grid(i, j)

    @_lib.serialized
    def fit_grid(self, grid_name, data_name, dof='ndata', offset=True):
        """Rank every model of ``grid_name`` against ``data_name`` (reference analyze.py:305-388): the models binned to
        the data (``mean_regrid``'s bits) in one launch, then per model the offset (when ``offset``: the mean of
        ``y_data - model``, what the reference's unweighted ``curve_fit`` of a constant converges to), the model plus
        offset and the reduced chi squared -- over ``len(data)`` when ``dof == 'ndata'``, else over ``len(data)`` less
        the number of grid parameters.  Fills ``chi_sqs``, ``best_fits``, ``offsets``, ``rank`` and ``posteriors``
        ``[grid_name][data_name]``."""
        dev = self._device(grid_name)
        ctx, nmodels = dev["ctx"], dev["nrows"]
        y_data, e_data = self.data[data_name]['y_data'], self.data[data_name]['e_data']
        numparams = self.overview[grid_name]['num_params']
        if dof == 'ndata':
            numparams = 0
        plan = self._plan(grid_name, data_name)
        one = np.ones(nmodels)
        binned = grid_rows(ctx, dev["spectra"], nmodels, dev["nwave"], np.arange(nmodels, dtype=np.int32)[:, None],
                           one[:, None], np.ones(nmodels, dtype=np.int32), one, plan=plan)
        shift, chi2, best = grid_chi2(ctx, binned, nmodels, y_data, e_data, offset, numparams)
        for name in ('chi_sqs', 'best_fits', 'rank', 'posteriors', 'offsets'):
            table = getattr(self, name, None)
            if table is None:
                table = {}
                setattr(self, name, table)
            table.setdefault(grid_name, {})
        self.chi_sqs[grid_name][data_name] = chi2
        self.best_fits[grid_name][data_name] = best
        self.offsets[grid_name][data_name] = shift
        self.rank[grid_name][data_name] = chi2.argsort()
        self.posteriors[grid_name][data_name] = {}
        for iattr in self.grid_params[grid_name].keys():
            for ikey in self.grid_params[grid_name][iattr].keys():
                self.posteriors[grid_name][data_name][ikey] = self.get_chi_posteriors(grid_name, data_name, ikey)

    def print_best_fit(self, grid_name, data_name, verbose=True):
        best_fits = {}
        for iattr in self.grid_params[grid_name].keys():
            for ikey in self.grid_params[grid_name][iattr].keys():
                single_best_fit = self.grid_params[grid_name][iattr][ikey][self.rank[grid_name][data_name]][0]
                if verbose:
                    print(f'{ikey}={single_best_fit}')
                best_fits[ikey] = single_best_fit
        return best_fits

    def get_chi_posteriors(self, grid_name, data_name, parameter):
        """``(unique values of the parameter, probability of each)`` from ``exp(-chi2 / 2)``, normalised over the grid
        (reference analyze.py:515-546)."""
        parameter_sort = _finditem(self.grid_params[grid_name], parameter)
        if isinstance(parameter_sort, type(None)):
            raise Exception(f'Parameter {parameter} not found in grid {grid_name}')
        chi_sq = self.chi_sqs[grid_name][data_name]
        parameter_grid = np.unique(parameter_sort)
        prob_array = np.exp(-chi_sq / 2.0)
        alpha = 1.0 / np.sum(prob_array)
        prob_array = prob_array * alpha
        prob = np.array([])
        for m in parameter_grid:
            wh = np.where(parameter_sort == m)
            prob = np.append(prob, np.sum(prob_array[wh]))
        return parameter_grid, prob

    def prep_gridtrieval(self, grid_name):
        """Prepare ``grid_name`` for interpolation between its nodes: the square-grid part of the reference's
        ``transform_4_interp`` (analyze.py:730-812).  ``interp_params[grid_name]`` gets ``grid_parameters_unique``
        (sorted unique values per parameter, in ``grid_params`` order), ``grid_parameters`` (every model's values),
        ``offset_prior`` and, built when first read, ``square_spectra_grid`` (NaN where the grid has no model).  What the
        device path reads instead of that array is ``node_rows``: the model row of every node, -1 for a missing
        combination or a row with NaN; of several models on one node the first counts."""
        spectra = self.spectra[grid_name]
        names, cols = [], []
        for i in self.grid_params[grid_name].keys():
            for j in self.grid_params[grid_name][i].keys():
                names.append(j)
                cols.append(np.asarray(self.grid_params[grid_name][i][j], dtype=float))
        if not names:
            raise Exception("prep_gridtrieval: grid %r has no parameters" % grid_name)
        points = np.stack(cols, axis=1)
        uniq = {n: np.unique(c) for n, c in zip(names, cols)}
        shape = tuple(len(u) for u in uniq.values())
        flat = np.ravel_multi_index(tuple(np.searchsorted(uniq[n], c) for n, c in zip(names, cols)), shape)
        nodes, first = np.unique(flat, return_index=True)
        node_rows = np.full(int(np.prod(shape)), -1, dtype=np.int64)
        node_rows[nodes] = np.where(self._dev[grid_name]["missing"][first], -1, first)
        offset_pm = abs(2 * (np.min(spectra) - np.max(spectra)))
        try:
            import pandas as pd
            table = pd.DataFrame({n: c for n, c in zip(names, cols)})
        except ImportError:
            table = {n: c for n, c in zip(names, cols)}
        ip = _InterpParams()
        ip['offset_prior'] = offset_pm
        ip['grid_parameters'] = table
        ip['grid_parameters_unique'] = uniq
        ip['node_rows'] = node_rows.reshape(shape)
        ip['_points'] = points
        ip['_spectra'] = spectra
        self.interp_params[grid_name] = ip


# ---------------------------------------------------------------------------------------------- interpolation
def _cell(names, pars, goals):
    """Per parameter the lower node index ``j`` (S, d) and the weight of the upper node ``w`` (S, d) of every goal, as
    ``find_bounding_values`` and ``custom_interp`` form them."""
    goals = np.atleast_2d(np.asarray(goals, dtype=float))
    d = len(pars)
    if goals.ndim != 2 or goals.shape[1] != d:
        raise Exception("custom_interp: a goal holds one value per grid parameter (%s), got shape %s"
                        % (", ".join(names), goals.shape))
    if d > MAX_DIM:
        raise Exception("custom_interp: %d parameters (%s); at most %d (2^%d = %d corners per sample)"
                        % (d, ", ".join(names), MAX_DIM, MAX_DIM, MAX_K))
    S = goals.shape[0]
    j, w = np.empty((S, d), dtype=np.int64), np.empty((S, d))
    for p, (name, arr) in enumerate(zip(names, pars)):
        if len(arr) < 2:
            raise Exception("custom_interp: parameter %s has the single value %s; interpolation needs two nodes at least"
                            % (name, arr[0] if len(arr) else None))
        v = goals[:, p]
        if not np.all(v >= arr[0]):
            raise Exception("custom_interp: %s = %s is below the grid (or NaN); the grid's range is [%s, %s]"
                            % (name, v[~(v >= arr[0])][0], arr[0], arr[-1]))
        jp = np.minimum(np.searchsorted(arr, v, side="right") - 1, len(arr) - 2)   # the last arr[j] <= v, clamped
        j[:, p] = jp
        w[:, p] = (v - arr[jp]) / (arr[jp + 1] - arr[jp])
    return goals, j, w


def interp_tables(goals, fitter, grid_name):
    """The tables of ``picaso_grid_rows_dev`` for the goals ``(S, d)``: ``rows`` (S, K) int32, ``wts`` (S, K), ``kcount``
    (S) int32 and ``div`` (S), ``K = 2^d`` (3 at least where a sample takes the fallback).

    Corners run in ``itertools.product([0, 1], repeat=d)`` order, the first parameter slowest; a corner's weight is the
    left-to-right product of its ``d`` factors ``1 - w`` / ``w`` (``np.prod`` of the reference's list).  A value at or
    above a parameter's last node uses its last two nodes (and extrapolates), as the reference does.  A sample with a
    corner on a missing node takes the reference's fallback (analyze.py:994-998): the three nearest existing models in
    raw parameter space, weights ``1 / dd**2``, divided by ``np.sum`` of the weights -- a sample exactly on an existing
    model (``dd = 0``) is NaN, as there."""
    ip = _interp_params(fitter, grid_name)
    uniq = ip['grid_parameters_unique']
    names, pars = list(uniq.keys()), list(uniq.values())
    goals, j, w = _cell(names, pars, goals)
    S, d = goals.shape
    node_rows = ip['node_rows']
    ncorner = 2 ** d
    K = max(ncorner, 3) if np.any(node_rows < 0) else ncorner
    rows, wts = np.zeros((S, K), dtype=np.int32), np.zeros((S, K))
    kcount, div = np.full(S, ncorner, dtype=np.int32), np.ones(S)
    inv = 1 - w
    for c, bits in enumerate(itertools.product([0, 1], repeat=d)):
        cw = None
        for p, b in enumerate(bits):
            f = w[:, p] if b else inv[:, p]
            cw = f if cw is None else cw * f
        rows[:, c] = node_rows[tuple(j[:, p] + b for p, b in enumerate(bits))]
        wts[:, c] = cw
    holes = np.flatnonzero(np.any(rows[:, :ncorner] < 0, axis=1))
    if holes.size:
        have = np.flatnonzero(~fitter._dev[grid_name]["missing"])
        if have.size < 3:
            raise Exception("custom_interp: the fallback for a missing node needs three models, grid %r has %d"
                            % (grid_name, have.size))
        pts = ip['_points'][have]
        dd = np.sqrt(np.sum((pts[None, :, :] - goals[holes][:, None, :]) ** 2, axis=2))
        near = np.argsort(dd, axis=1, kind="stable")[:, :3]
        with np.errstate(divide="ignore"):
            wn = 1.0 / np.take_along_axis(dd, near, axis=1) ** 2
        rows[holes], wts[holes] = 0, 0.0
        rows[holes, :3], wts[holes, :3] = have[near], wn
        kcount[holes] = 3
        div[holes] = np.sum(wn, axis=1)
    return rows, wts, kcount, div


def _interp_params(fitter, grid_name):
    ip = fitter.interp_params.get(grid_name)
    if ip is None:
        raise Exception("grid %r is not prepared: call fitter.prep_gridtrieval(%r) first" % (grid_name, grid_name))
    return ip


@_lib.serialized
def interp_batch(goals, fitter, grid_name):
    """``custom_interp`` of the spectra for every goal of ``goals`` (S, d) in one launch: (S, nwave), each row bit for
    bit what the reference's ``custom_interp`` returns for it (on a grid without missing nodes; the fallback's sum is
    taken in table order, the reference's in its BLAS's)."""
    tables = interp_tables(goals, fitter, grid_name)
    dev = fitter._device(grid_name)
    out = grid_rows(dev["ctx"], dev["spectra"], dev["nrows"], dev["nwave"], *tables, full=True).to_host()
    return np.ascontiguousarray(out[:, ::-1]) if dev["flip"] else out


@_lib.serialized
def loglike_batch(goals, fitter, grid_name, data_name, offset=0, scaling=1, err_inf=0, return_binned=False):
    """The retrieval's log likelihood (reference driver.py:296-326) of the spectra interpolated to ``goals`` (S, d) and
    binned to ``data_name``: ``-0.5 * sum(((y + offset) * scaling - model)**2 / (e**2 + err_inf) + log(2 pi (e**2 +
    err_inf)))`` per sample, (S,).  ``offset`` / ``scaling`` / ``err_inf``: a scalar or (S,).  Interpolation and binning
    are one launch: the interpolated spectra never reach memory.  ``return_binned``: also the (S, ndata) binned models,
    ``mean_regrid`` of ``custom_interp`` bit for bit."""
    rows, wts, kcount, div = interp_tables(goals, fitter, grid_name)
    dev = fitter._device(grid_name)
    ctx = dev["ctx"]
    S = rows.shape[0]
    for nm, v in (("offset", offset), ("scaling", scaling), ("err_inf", err_inf)):
        if np.ndim(v) > 1 or (np.ndim(v) == 1 and np.shape(v) != (S,)):
            raise Exception("loglike_batch: %s must be a scalar or (%d,), got shape %s" % (nm, S, np.shape(v)))
    binned = grid_rows(ctx, dev["spectra"], dev["nrows"], dev["nwave"], rows, wts, kcount, div,
                       plan=fitter._plan(grid_name, data_name))
    data = fitter.data[data_name]
    logl = grid_loglike(ctx, binned, S, data['y_data'], data['e_data'], offset, scaling, err_inf)
    return (logl, binned.to_host()) if return_binned else logl


@_lib.serialized
def bands_batch(goals, fitter, grid_name, data_name=None, q=None):
    """The prediction bands of a gridtrieval: the quantile lines ``q`` (levels or a dictionary of them; default
    ``retrieval.SIGMA_QUANTILES``, the reference's seven) over the spectra interpolated to the posterior draws ``goals``
    (S, d) -- ``retrieval.bands(interp_batch(goals, ...), q)`` bit for bit, (len(q), nwave), or with ``data_name`` the
    bands of the spectra binned to that data set, ``bands`` of ``loglike_batch(..., return_binned=True)[1]``,
    (len(q), ndata).  The interpolated spectra stay in HBM: ``picaso_column_quantiles_dev`` reads them there and only the
    lines come back."""
    from . import retrieval
    p = retrieval._levels(retrieval.SIGMA_QUANTILES if q is None else q)
    if not 1 <= p.size <= retrieval.MAX_Q:
        raise Exception("bands_batch: %d levels; one call takes 1 to %d" % (p.size, retrieval.MAX_Q))
    tables = interp_tables(goals, fitter, grid_name)
    S = tables[0].shape[0]
    if S > retrieval.MAX_DRAWS:
        raise Exception("bands_batch: %d draws; a column is sorted in LDS and takes at most %d" % (S, retrieval.MAX_DRAWS))
    k, gamma = retrieval.quantile_table(S, p)
    dev = fitter._device(grid_name)
    if data_name is None:
        stack = grid_rows(dev["ctx"], dev["spectra"], dev["nrows"], dev["nwave"], *tables, full=True)
    else:
        stack = grid_rows(dev["ctx"], dev["spectra"], dev["nrows"], dev["nwave"], *tables,
                          plan=fitter._plan(grid_name, data_name))
    out = retrieval.column_quantiles(stack, k, gamma).to_host()
    return np.ascontiguousarray(out[:, ::-1]) if data_name is None and dev["flip"] else out


def custom_interp(final_goal, fitter, grid_name, to_interp='spectra', array_to_interp=None):
    """Interpolate linearly between the two nearest nodes of every grid parameter (reference analyze.py:923-1000).

    ``final_goal``: one value per parameter in ``grid_parameters_unique`` order.  ``to_interp='spectra'``: the spectrum,
    through the device (``interp_batch`` of one sample).  Anything else: ``array_to_interp``, an array on the square
    grid's leading axes with any last axis (temperatures, abundances), on the host."""
    if 'spectra' in to_interp:
        return interp_batch(np.asarray(final_goal, dtype=float)[None, :], fitter, grid_name)[0]
    ip = _interp_params(fitter, grid_name)
    uniq = ip['grid_parameters_unique']
    goals, j, w = _cell(list(uniq.keys()), list(uniq.values()), final_goal)
    if goals.shape[0] != 1:
        raise Exception("custom_interp: one goal at a time; interp_batch takes many")
    all_weights = np.array([1 - w[0], w[0]]).T
    interp = 0
    for irow in itertools.product([0, 1], repeat=goals.shape[1]):
        weight_multip = [all_weights[i][b] for i, b in enumerate(irow)]
        inds = [int(j[0, i]) + b for i, b in enumerate(irow)] + [-1]
        interp += np.prod(weight_multip) * get_last_dimension(array_to_interp, inds)
    return interp
