"""Equilibrium chemistry from tables: the Visscher grids, their loaders, and the batched interpolation on the device.

The reference interpolates a chemistry table one profile at a time (justdoit.py:3106-3199, ``chem_interp``) and, for a 3-D
run, once per (lon, lat) column in a joblib pool, re-reading the grid file for every column (justdoit.py:3517-3664,
``premix_3d`` / ``chemeq_3d``).  Here the table is resident (``ChemTable``: log10 of the abundances as one row-major matrix,
uploaded once and memoised by content) and ``chem_interp_batch`` interpolates every species at every point of any number of
columns in ONE launch of ``picaso_chem_interp_dev`` (csrc/cheminterp.hip).

``interp_numpy`` is the numpy form, the body ``inputs.chem_interp`` has always had; the device exponent equals its exponent
bit for bit and the abundance ``10**x`` lies within 4 ulp of numpy's.

Loaders return a dictionary of columns -- ``pressure`` (bar), ``temperature`` (K), one array per species in file order --
the form ``inputs.chem_interp`` and ``ChemTable`` take.  The 1-D route: ``case.chem_interp(chemistry.visscher_2121(0.55,
0.0))``.
"""
import math
import os
import re

import numpy as np

from . import _lib
from .device import DeviceArray

NOT_SPECIES = ("pressure", "temperature")


# ---------------------------------------------------------------------------------------------------------------------
# readers
# ---------------------------------------------------------------------------------------------------------------------
def _read_rows(filename, sep):
    """The rows below the header line as a float64 matrix: with pandas' float parser where pandas is there, as the reference
    reads them (its last bit can differ from strtod's), else with numpy's."""
    try:
        import pandas as pd
        return pd.read_csv(filename, sep=sep, skiprows=1, header=None).values.astype(np.float64)
    except ImportError:
        return np.loadtxt(filename, dtype=np.float64, skiprows=1, ndmin=2, delimiter=None if sep != "," else ",")


def _read_visscher(filename, t_name, p_name):
    with open(filename) as fh:
        header = fh.readline()
    cols = header.replace(t_name, "temperature").replace(p_name, "pressure").split()
    data = _read_rows(filename, r"\s+")
    if data.shape[1] != len(cols):
        raise ValueError("%s: the header names %d columns, the rows hold %d" % (filename, len(cols), data.shape[1]))
    out = {k: np.ascontiguousarray(data[:, i]) for i, k in enumerate(cols)}
    out["pressure"] = 10 ** out["pressure"]
    return out


def read_visscher_2121(filename):
    """One file of the 2121-point grid as a dictionary of columns (reference io_utils.py:7-24, ``read_visscher_2121``): a
    header line with ``T(K)``, ``P(bar)`` and the species names, whitespace-separated rows, ``pressure = 10**column``."""
    return _read_visscher(filename, "T(K)", "P(bar)")


def read_visscher_1060(filename):
    """One file of the 1060-point grid (reference justdoit.py:3084-3087): as ``read_visscher_2121`` with the header spelling
    ``T (K)``, ``P (bar)``."""
    return _read_visscher(filename, "T (K)", "P (bar)")


def read_channon_grid_low(filename):
    """``chemistry/visscher_abunds_m+0.0_co1.0`` (reference justdoit.py:3101-3103): a CSV whose first column is an index,
    which is dropped; ``pressure`` is in bar as it stands."""
    with open(filename) as fh:
        cols = fh.readline().rstrip("\r\n").split(",")
    data = _read_rows(filename, ",")
    if data.shape[1] != len(cols):
        raise ValueError("%s: the header names %d columns, the rows hold %d" % (filename, len(cols), data.shape[1]))
    return {k: np.ascontiguousarray(data[:, i]) for i, k in enumerate(cols) if i > 0}


def _refdata():
    ref = os.environ.get("picaso_refdata")
    if not ref:
        raise FileNotFoundError("the chemistry grids are looked up under $picaso_refdata/chemistry, and picaso_refdata is not "
                                "set: set it, or name the directory")
    return ref


_FLOAT = r"[-+]?(?:\d+\.?\d*|\.\d+)"                                  # the reference's pattern (justdoit.py:2942)
_FILE_2121 = re.compile(r"sonora_2121grid_feh(%s)_co(%s)\.txt" % (_FLOAT, _FLOAT))


def select_visscher_2121(cto_absolute, log_mh, directory=None):
    """The file of the 2121 grid nearest to ``(log_mh, cto_absolute)``, as the reference chooses it (justdoit.py:2924-3006):
    every ``sonora_2121grid_feh<f>_co<c>.txt`` of the directory is a candidate, the smallest Euclidean distance in (feh, co)
    wins, a tie goes to the smaller ``|dfeh|``, then to the smaller ``|dco|``.

    One difference: candidates that still tie are taken in SORTED filename order (the first wins); the reference takes them
    in ``os.listdir`` order, which depends on the file system.  Returns the full path."""
    if directory is None:
        directory = os.path.join(_refdata(), "chemistry", "visscher_grid_2121")
    if not os.path.isdir(directory):
        raise FileNotFoundError("Directory not found: %s" % directory)
    best = None
    for filename in sorted(os.listdir(directory)):
        m = _FILE_2121.match(filename)
        if not m:
            continue
        dfeh, dco = float(m.group(1)) - log_mh, float(m.group(2)) - cto_absolute
        key = (math.sqrt(dfeh ** 2 + dco ** 2), abs(dfeh), abs(dco))
        if best is None or key < best[0]:
            best = (key, filename)
    if best is None:
        raise Exception("No files matching the pattern '%s' found in directory '%s'." % (_FILE_2121.pattern, directory))
    return os.path.join(directory, best[1])


def visscher_2121(cto_absolute, log_mh, directory=None):
    """The table of the 2121 grid nearest to ``cto_absolute`` (solar 0.55) and ``log_mh`` (solar 0): what the reference's
    ``chemeq_visscher_2121`` hands to ``chem_interp`` (justdoit.py:2924-3026).  ``directory=None``:
    ``$picaso_refdata/chemistry/visscher_grid_2121``; a missing directory is a ``FileNotFoundError`` naming it.  The choice of
    the file and its one difference from the reference: ``select_visscher_2121``."""
    return read_visscher_2121(select_visscher_2121(cto_absolute, log_mh, directory))


def select_visscher_1060(c_o, log_mh, directory=None):
    """The file of the 1060 grid for ``c_o`` (relative to solar) and ``log_mh`` (reference justdoit.py:3066-3082): the nearest
    of the allowed values of each, and the reference's two exceptions above them."""
    cos = np.array([0.25, 0.5, 1.0, 1.5, 2.0, 2.5])
    fehs = np.array([-0.3, 0.0, 0.3, 0.5, 0.7, 1.0, 1.5, 1.7, 2.0])
    if log_mh > max(fehs):
        raise Exception('Choose a log metallicity less than 2.0')
    if c_o > max(cos):
        raise Exception('Choose a C/O less than 2.5xSolar')
    grid_co = cos[np.argmin(np.abs(cos - c_o))]
    grid_feh = fehs[np.argmin(np.abs(fehs - log_mh))]
    str_co = str(grid_co).replace('.', '')
    str_fe = str(grid_feh).replace('.', '').replace('-', 'm')
    if directory is None:
        directory = os.path.join(_refdata(), "chemistry", "visscher_grid_1060")
    return os.path.join(directory, '2015_06_1060grid_feh_%s_co_%s.txt' % (str_fe, str_co)).replace('_m0', 'm0')


def visscher_1060(c_o, log_mh, directory=None):
    """The table of the 1060 grid nearest to ``c_o`` (relative to solar) and ``log_mh``: what the reference's
    ``chemeq_visscher_1060`` hands to ``chem_interp`` (justdoit.py:3066-3090).  ``directory=None``:
    ``$picaso_refdata/chemistry/visscher_grid_1060``."""
    return read_visscher_1060(select_visscher_1060(c_o, log_mh, directory))


# ---------------------------------------------------------------------------------------------------------------------
# the numpy form
# ---------------------------------------------------------------------------------------------------------------------
def table_grids(chem_grid):
    """What ``chem_interp`` derives from a table (reference justdoit.py:3116-3140): the species in column order, log10 of
    their abundances ``(nrow, nspecies)``, ``t_inv_grid``, ``p_log_grid``, the pressure count ``nc_p`` of every temperature
    and the first row ``start`` of every temperature (one entry more than there are temperatures)."""
    tab_t, tab_p = np.asarray(chem_grid["temperature"], dtype=float), np.asarray(chem_grid["pressure"], dtype=float)
    species = [k for k in chem_grid.keys() if k not in NOT_SPECIES]
    with np.errstate(divide="ignore"):
        log_abunds = np.log10(np.stack([np.asarray(chem_grid[k], dtype=float) for k in species], axis=1))
    nc_p = np.unique(tab_t, return_counts=True)[1]               # per temperature, in ascending temperature
    _, first = np.unique(tab_t, return_index=True)
    temps = tab_t[np.sort(first)]                                # in order of appearance, as the reference reads them
    p_grid = np.unique(tab_p)
    p_log_grid = np.log10(p_grid[p_grid > 0])
    t_inv_grid = 1 / temps
    start = np.concatenate(([0], np.cumsum(nc_p)))               # first row of every temperature
    return species, log_abunds, t_inv_grid, p_log_grid, nc_p, start


def interp_numpy(temperature, pressure, chem_grid, log10=False):
    """Abundances at the points ``(temperature, pressure)`` (1-D arrays of one length) from the table ``chem_grid``: the body
    of ``inputs.chem_interp`` (reference justdoit.py:3106-3199), bilinear in ``(1/T, log10 P)`` of the log10 abundance.
    Returns ``(species, abunds)``, ``abunds`` ``(npoints, nspecies)``; ``log10=True``: the exponent ``x`` of ``10**x``
    instead.  This is the yardstick of the device kernel."""
    plevel, tlevel = np.asarray(pressure, dtype=float), np.asarray(temperature, dtype=float)
    t_inv, p_log = 1 / tlevel, np.log10(plevel)
    species, log_abunds, t_inv_grid, p_log_grid, nc_p, start = table_grids(chem_grid)
    nt = len(t_inv_grid)

    def last_where(mask):                                        # last true index of every row, 0 when none
        idx = mask.shape[1] - 1 - np.argmax(mask[:, ::-1], axis=1)
        return np.where(mask.any(axis=1), idx, 0)
    t_low = last_where(t_inv_grid[None, :] > t_inv[:, None])
    t_low[t_low == nt - 1] = nt - 2
    t_hi = t_low + 1
    p_low = np.minimum(last_where(p_log_grid[None, :] <= p_log[:, None]), nc_p[t_hi] - 3)
    p_hi = p_low + 1
    t_i = ((t_inv - t_inv_grid[t_low]) / (t_inv_grid[t_hi] - t_inv_grid[t_low]))[:, None]
    p_i = ((p_log - p_log_grid[p_low]) / (p_log_grid[p_hi] - p_log_grid[p_low]))[:, None]
    x = (((1 - t_i) * (1 - p_i) * log_abunds[start[t_low] + p_low, :])
         + (t_i * (1 - p_i) * log_abunds[start[t_hi] + p_low, :])
         + (t_i * p_i * log_abunds[start[t_hi] + p_hi, :])
         + ((1 - t_i) * p_i * log_abunds[start[t_low] + p_hi, :]))
    if log10:
        return species, x
    return species, 10 ** x


# ---------------------------------------------------------------------------------------------------------------------
# the resident table
# ---------------------------------------------------------------------------------------------------------------------
_tables = {}            # (pid, context, digest of the table) -> ChemTable: content-addressed, oldest out first
_TABLES_MAX = 16
UPLOADS = 0             # tables uploaded by this process so far (a memo hit does not count)
_lib.on_context_destroy(lambda value: [_tables.pop(k) for k in [k for k in _tables if k[1] == value]])


def clear_table_cache():
    """Drop the resident chemistry tables kept by ``ChemTable.resident``."""
    _tables.clear()


def _upload_i32(a, ctx):
    """int32 values in HBM, carried by a float64 DeviceArray of the same bytes (as ``analyze._upload_i32``)."""
    a = np.ascontiguousarray(a, dtype=np.int32).ravel()
    padded = np.zeros((a.size + 1) // 2 * 2, dtype=np.int32)
    padded[:a.size] = a
    return DeviceArray.from_host(padded.view(np.float64), ctx)


class ChemTable(object):
    """A chemistry table resident in HBM: log10 of the abundances as one ``(nrow, nspecies)`` row-major matrix, with
    ``t_inv_grid``, ``p_log_grid``, ``nc_p`` and the first row of every temperature, all formed as ``inputs.chem_interp``
    forms them (``table_grids``; ``np.log10`` runs on the host, once).

    Refused with a ``ValueError``: fewer than two temperatures, fewer than two positive pressures, a temperature with fewer
    than three pressures (``nc_p - 3`` is a row offset), a temperature with more rows than there are positive pressures, and a
    row count other than ``sum(nc_p)``.  With those checks every row the kernel's clamps can produce lies inside the matrix:
    ``p_low`` is in ``[0, nc_p[t_hi] - 3]``, so the largest row is ``start[t_hi] + nc_p[t_hi] - 2 < nrow`` and the largest
    pressure index ``nc_p[t_hi] - 2 < npres``.

    ``ChemTable.resident(columns, ctx)`` memoises by content: the same table, from the same file or the same
    ``opa.full_abunds``, is uploaded once per context."""

    def __init__(self, columns, ctx=None):
        global UPLOADS
        for key in NOT_SPECIES:
            if key not in columns.keys():
                raise ValueError("chemistry table: no %r column" % key)
        if not [k for k in columns.keys() if k not in NOT_SPECIES]:
            raise ValueError("chemistry table: no species columns")
        species, log_abunds, t_inv_grid, p_log_grid, nc_p, start = table_grids(columns)
        if len(t_inv_grid) < 2:
            raise ValueError("chemistry table: %d temperature(s); the interpolation needs two" % len(t_inv_grid))
        if len(p_log_grid) < 2:
            raise ValueError("chemistry table: %d positive pressure(s); the interpolation needs two" % len(p_log_grid))
        if np.any(nc_p < 3):
            raise ValueError("chemistry table: a temperature with %d pressure(s); every temperature needs three (the lower "
                             "pressure index is held to nc_p - 3)" % int(nc_p.min()))
        if np.any(nc_p > len(p_log_grid)):
            raise ValueError("chemistry table: a temperature with %d rows, but only %d positive pressures"
                             % (int(nc_p.max()), len(p_log_grid)))
        if log_abunds.shape[0] != int(nc_p.sum()):
            raise ValueError("chemistry table: %d rows, but the pressure counts of its temperatures add up to %d"
                             % (log_abunds.shape[0], int(nc_p.sum())))
        self.ctx = ctx if ctx is not None else _lib.context()
        self.species = list(species)
        self.nrow, self.nspecies = log_abunds.shape
        self.ntemp, self.npres = len(t_inv_grid), len(p_log_grid)
        self.host = dict(t_inv_grid=t_inv_grid, p_log_grid=p_log_grid, nc_p=nc_p, start=start)
        self.d_log_abunds = DeviceArray.from_host(log_abunds, self.ctx)
        self.d_grids = DeviceArray.from_host(np.concatenate([t_inv_grid, p_log_grid]), self.ctx)
        self.d_ints = _upload_i32(np.concatenate([nc_p, start[:-1]]), self.ctx)
        UPLOADS += 1

    @classmethod
    def resident(cls, columns, ctx=None):
        """The resident form of ``columns`` (a ``ChemTable`` is returned as it is), from the memo when a table of the same
        content is already there."""
        if isinstance(columns, cls):
            return columns
        from .optics import content_digest
        ctx = ctx if ctx is not None else _lib.context()
        stamp = tuple((str(k), content_digest(np.asarray(columns[k], dtype=np.float64))) for k in columns.keys())
        key = (os.getpid(), getattr(ctx, "value", ctx), stamp)
        hit = _tables.get(key)
        if hit is None:
            while len(_tables) >= _TABLES_MAX:
                del _tables[next(iter(_tables))]
            hit = _tables[key] = cls(columns, ctx)
        return hit


def chem_interp_dev(table, d_temperature, d_p_log, npoints, sel=None, log10=False):
    """``picaso_chem_interp_dev`` on resident points: ``d_temperature`` and ``d_p_log`` are DeviceArrays of ``npoints``
    values, ``sel`` a sequence of column indices of the table (``None``: all).  Returns the ``(nsel, npoints)`` DeviceArray;
    the launch is asynchronous and the result keeps its inputs alive."""
    ctx = table.ctx
    if sel is None:
        nsel, d_sel = table.nspecies, None
    else:
        sel = np.ascontiguousarray(sel, dtype=np.int32)
        if sel.ndim != 1 or sel.size < 1 or sel.min() < 0 or sel.max() >= table.nspecies:
            raise _lib.PicasoHipError("chem_interp_dev: the selection must be 1-D, non-empty and inside [0, %d)" % table.nspecies)
        nsel, d_sel = sel.size, _upload_i32(sel, ctx)
    out = DeviceArray((nsel, int(npoints)), ctx)
    _lib.check(_lib.load().picaso_chem_interp_dev(
        ctx, table.nrow, table.nspecies, table.d_log_abunds.addr, table.ntemp, table.npres, table.d_grids.addr,
        table.d_grids.addr + 8 * table.ntemp, table.d_ints.addr, table.d_ints.addr + 4 * table.ntemp, int(npoints),
        d_temperature.addr, d_p_log.addr, nsel, _lib.addr(d_sel), int(bool(log10)), out.addr), ctx)
    out._inputs = (table, d_temperature, d_p_log, d_sel)
    return out


@_lib.serialized
def chem_interp_batch(temperature, pressure, table, species=None, log10=False, out="host", ctx=None):
    """Every species of ``table`` at every point ``(temperature, pressure)`` in one launch (the batched form of the
    reference's ``chem_interp``, justdoit.py:3106-3199, and of the per-column pool of ``chemeq_3d``, :3590-3664).

    ``temperature`` (K) and ``pressure`` (bar): arrays of one shape, any rank.  ``table``: a ``ChemTable`` or a dictionary of
    columns (made resident, memoised by content).  ``species``: a subset in the caller's order (default: all, in table
    order).  Returns ``{species: array of the input shape}``; ``log10=True`` gives the interpolated exponent instead of the
    abundance.  ``out="device"`` returns ``(DeviceArray (nspecies, npoints), [species])`` and copies nothing back.  Zero points
    give empty arrays and no launch (``out="device"``: ``(None, [species])``).

    ``log10 P`` is taken here, on the host and on a contiguous copy, so that the exponent has the bits ``interp_numpy`` gives
    for contiguous arrays."""
    if out not in ("host", "device"):
        raise ValueError("chem_interp_batch: out must be 'host' or 'device', got %r" % (out,))
    # contiguous copies: numpy's log10 takes another loop for a strided array, whose last bit can differ, and a point's
    # result must not depend on how the caller's array is laid out
    t = np.require(temperature, np.float64, "C")
    p = np.require(pressure, np.float64, "C")
    if t.shape != p.shape:
        raise ValueError("chem_interp_batch: temperature has shape %s, pressure %s" % (t.shape, p.shape))
    tab = ChemTable.resident(table, ctx)
    if species is None:
        names, sel = list(tab.species), None
    else:
        names = [species] if isinstance(species, str) else list(species)
        missing = [s for s in names if s not in tab.species]
        if missing:
            raise KeyError("chem_interp_batch: the table has no species %s" % ", ".join(map(str, missing)))
        if not names:
            raise ValueError("chem_interp_batch: an empty species list")
        sel = [tab.species.index(s) for s in names]
    if t.size == 0:
        if out == "device":
            return None, names
        return {s: np.empty(t.shape) for s in names}
    with np.errstate(divide="ignore", invalid="ignore"):
        p_log = np.log10(p)
    d_t = DeviceArray.from_host(t.reshape(-1), tab.ctx)
    d_p = DeviceArray.from_host(p_log.reshape(-1), tab.ctx)
    d_out = chem_interp_dev(tab, d_t, d_p, t.size, sel, log10)
    if out == "device":
        return d_out, names
    host = d_out.to_host()
    return {s: host[i].reshape(t.shape) for i, s in enumerate(names)}
