"""Correlated-k tables from line-by-line cross sections on the device: ``jdi.compute_ck`` and ``jdi.compute_ck_molecular``.

The tables ``read_ck_tables`` reads and ``RetrieveCKs`` keeps in HBM are made by the reference's
``opacity_factory.compute_ck_molecular`` (opacity_factory.py:1748-2008): for every P-T point of a cross-section directory
and every bin of the new wavenumber grid it sorts the logarithms of the line-by-line points that fall in the bin and reads
the sorted curve at the Gauss abscissae with ``np.interp`` (:1927-1955), in Python, one bin at a time.  Here the bins of a row
become segments ``[lo, lo + n)`` of it on the host (``ck_segments``: the reference's membership test on the numpy-built
grid, so a point exactly on an edge never depends on device arithmetic), the row is uploaded once, and one launch of
``picaso_ck_from_xsec_dev`` (csrc/ckfactory.hip) selects the two order statistics each Gauss point needs in every bin -- an
LDS sort for short segments, a radix multi-select from HBM for long ones -- and interpolates their logarithms in numpy's
operation order.  The upload of the next row overlaps the kernels of the current one; only the table comes back.

``compute_ck``, the weighted sums and ``insert_molecular_1460`` are consumers of ONE row pipeline, ``_UploadRing.run``: it
alone stages a row ahead, orders the streams, waits before a slot is used again, checks a row's length against its grid and
tears down; it holds the one bounded cache of device grids (``_DeviceGrids``: validated, with the uniform-grid guess).

A PREMIXED table (one ``ln kappa`` for a gas mixture at one chemistry, what ``opannection(method="preweighted")`` and the
climate solver run on) is the same binning of the abundance-weighted sum of the gases' rows, the reference's
``compute_sum_molecular`` (:1530-1718) followed by the ``sum_<i>`` branch of ``compute_ck_molecular``.
``jdi.compute_ck_premixed`` forms that sum in HBM (``picaso_xsec_axpy_dev``, csrc/xsecsum.hip: numpy's sum bit for bit) and
bins it there; ``jdi.weighted_sum`` is the array form of the sum, ``jdi.compute_sum_molecular`` writes the reference's
intermediate file, ``premix_abundances`` selects the abundances as the reference does.

The other file an opacity object needs, the sqlite DATABASE (``header``, ``molecular``, ``continuum``), is written here too:
``build_skeleton`` and the readers keep the reference's schema; ``restruct_continuum`` / ``restructure_opacity`` put the CIA
file and the other continuum sources on a new grid (``continuum_rows``: ``picaso_continuum_rows_dev``, csrc/contfactory.hip,
with an exact median filter; ``continuum_rows_numpy``: the reference's arithmetic on the host); ``insert_molecular_1460``
resamples cross-section rows (``picaso_xsec_resample_dev``).  DESIGN section 5q.
"""
import collections
import ctypes
import glob
import io
import math
import os
import sqlite3

import numpy as np

from . import _lib, optics
from .device import DeviceArray, PinnedArray
from .device import sync as _sync

_c_ll_p = ctypes.POINTER(ctypes.c_longlong)
ALKALIS = ("Na", "K", "Rb", "Cs", "Li")


def uniform_grid(numw, delwn, start):
    """The wavenumbers of a uniform cross-section row as the reference forms them, in numpy:
    ``np.arange(numw) * delwn + start`` (opacity_factory.py:1912)."""
    return np.arange(int(numw)) * float(delwn) + float(start)


def ck_segments(og_wvno_grid, wvno_low, wvno_high):
    """``(lo, n)`` int64 arrays, one entry per bin: the points ``og[lo:lo + n]`` of the ascending grid ``og_wvno_grid`` are
    those with ``(og > wvno_low) & (og <= wvno_high)``, the reference's membership test (opacity_factory.py:1931).  Both
    edges are searched with ``side='right'``: a point on a low edge is left out, one on a high edge is taken.  Bins may
    overlap, leave gaps or lie outside the grid (``n = 0``)."""
    og = np.asarray(og_wvno_grid, dtype=float)
    low, high = np.asarray(wvno_low, dtype=float), np.asarray(wvno_high, dtype=float)
    if og.ndim != 1:
        raise Exception("ck_segments: the cross-section grid must be a 1-D array")
    if low.ndim != 1 or low.shape != high.shape:
        raise Exception("ck_segments: wvno_low and wvno_high must be 1-D arrays of one length, got %s and %s"
                        % (low.shape, high.shape))
    if og.size > 1 and not np.all(og[1:] >= og[:-1]):
        raise Exception("ck_segments: the cross-section grid must be ascending in wavenumber")
    lo = np.searchsorted(og, low, side="right").astype(np.int64)
    hi = np.searchsorted(og, high, side="right").astype(np.int64)
    return lo, np.maximum(hi - lo, 0)


def ck_segments_uniform(numw, delwn, start, wvno_low, wvno_high):
    """``ck_segments`` on the uniform grid ``uniform_grid(numw, delwn, start)``: the grid is built in numpy and searched as
    an array, not solved for the edges, so edge points fall as they do in the reference."""
    return ck_segments(uniform_grid(numw, delwn, start), wvno_low, wvno_high)


def get_wvno_grid(filename, min_wavelength=None, max_wavelength=None, R=None):
    """``(wvno_low, wvno_high, wvno_new, dwni_new)`` of the bins of a new table (reference opacity_factory.py:1505-1528):
    from a two-column file of wavenumbers and bin widths, or -- ``filename=None`` -- on the constant-resolution grid
    ``create_grid(min_wavelength, max_wavelength, R)``, whose widths are the differences of neighbours (the first one
    repeated).  The edges lie half a width either side of every wavenumber."""
    if filename is not None:
        wvno_new, dwni_new = np.loadtxt(filename, usecols=[0, 1], unpack=True)
    else:
        from .justdoit import create_grid
        wvno_new = create_grid(min_wavelength, max_wavelength, R)
        d = np.diff(wvno_new)
        dwni_new = np.concatenate((d[:1], d))
    return 0.5 * (2 * wvno_new - dwni_new), 0.5 * (2 * wvno_new + dwni_new), wvno_new, dwni_new


def _rows_of(cxs):
    """``cxs`` as a sequence of rows: one 1-D array is one row."""
    if isinstance(cxs, np.ndarray):
        if cxs.ndim == 1:
            return [cxs]
        if cxs.ndim == 2:
            return cxs
        raise Exception("compute_ck: cxs must be one row or a sequence of rows, got an array of shape %s" % (cxs.shape,))
    if not hasattr(cxs, "__len__") or not hasattr(cxs, "__getitem__"):
        raise Exception("compute_ck: cxs must be one row or a sequence of rows")
    if len(cxs) and np.ndim(cxs[0]) == 0:
        return [np.asarray(cxs, dtype=float)]
    return cxs


class _Segments:
    """``on(og)``: ``(lo, n, grid length)`` of the bins ``(low, high]`` on the grid ``og``, found once per grid object."""

    def __init__(self, low, high):
        self.low, self.high, self.cache = low, high, {}

    def on(self, og):
        hit = self.cache.get(id(og))
        if hit is None or hit[0] is not og:
            if len(self.cache) > 8:
                self.cache.clear()
            lo, n = ck_segments(og, self.low, self.high)
            hit = self.cache[id(og)] = (og, np.ascontiguousarray(lo), np.ascontiguousarray(n), int(np.size(og)))
        return hit[1:]


# One row for _UploadRing.run: rows[index] is read when the row is staged; label names it in messages; expect is the length
# its wavenumber grid says it has, or None; tag is whatever the consumer wants back.
_Row = collections.namedtuple("_Row", "label rows index expect tag", defaults=(None,))


class _DeviceGrids:
    """Device copies of wavenumber grids, found by the identity of the host array (re-checked: an id can come back).
    ``get(g, what)``: ``(address, start, step)`` of ``g``, validated and uploaded when it is first met; knot ``j`` lies near
    ``start + j step``, the guess a uniform grid of this span gives the kernels (``step`` 0: none).  ``trim()`` drops all
    but the three used last; the ring calls it right after its wait, when no kernel reads them."""

    def __init__(self, ctx, who):
        self.ctx, self.who, self.held = ctx, who, {}        # id -> (host grid, DeviceArray, start, step), last used last

    def get(self, g, what):
        hit = self.held.pop(id(g), None)
        if hit is None or hit[0] is not g:
            a = np.asarray(g, dtype=float)
            if a.ndim != 1 or a.size < 2 or not np.all(a[1:] >= a[:-1]):
                raise Exception("%s: %s must be an ascending 1-D array of at least 2 wavenumbers" % (self.who, what))
            step = (float(a[-1]) - float(a[0])) / (a.size - 1)
            hit = (g, DeviceArray.from_host(a, self.ctx), float(a[0]), step if np.isfinite(step) and step > 0.0 else 0.0)
        self.held[id(g)] = hit
        return hit[1].addr, hit[2], hit[3]

    def trim(self, keep=3):
        while len(self.held) > keep:
            self.held.pop(next(iter(self.held)))[1].free()


class _UploadRing:
    """The row pipeline of ``compute_ck``, the weighted sums and ``insert_molecular_1460``: two pinned blocks and two device
    buffers that rows of cross sections travel through one at a time, and the device copies of their grids (``grids``).
    ``run(items, consume)``: ``items`` yields ``_Row``s; ``consume(row, d_row, n_row)`` enqueues, on the first context, what
    reads the ``n_row`` points of row ``k`` from the DeviceArray ``d_row``.  Everything else happens here, in this order:

        stage 0;  then per row k:  landed;  stage k + 1;  check row k's length;  consume k;  wait

    *stage* takes the next item (a row is read one ahead, never further), copies it into the pinned block of slot ``k & 1``
    and enqueues its transfer on the second context's stream.  *landed* orders the first context's stream behind the
    transfers enqueued so far (the host does not block).  *wait* synchronises the first context: whatever the consumer's
    last call was, the kernels that read slot ``k & 1`` -- and so the transfer out of its pinned block -- are over before row
    ``k + 2`` is staged into it, and only then are grid copies dropped.  However ``run`` ends (the loader, the check or the
    consumer may raise), both streams are waited for and then the slots and grids are freed: a ring runs once."""

    def __init__(self, ctx, aux, who):
        self.ctx, self.aux, self.who, self.lib = ctx, aux, who, _lib.load()
        self.pinned, self.devs, self.grids = [None, None], [None, None], _DeviceGrids(ctx, who)

    def _stage(self, k, item):
        if item is None:
            return None
        row = np.asarray(item.rows[item.index], dtype=float)
        if row.ndim != 1 or row.size < 1:
            raise Exception("%s: %s must be a non-empty 1-D array, got shape %s" % (self.who, item.label, row.shape))
        s = k & 1
        if self.pinned[s] is None or self.pinned[s].shape != row.shape:
            for old in (self.pinned[s], self.devs[s]):
                if old is not None:
                    old.free()
            self.pinned[s], self.devs[s] = PinnedArray(row.shape, self.aux), DeviceArray(row.shape, self.ctx)
        self.pinned[s].array[:] = row
        _lib.check(self.lib.picaso_memcpy_h2d_async(self.aux, self.devs[s].addr, self.pinned[s].addr, 8 * row.size), self.aux)
        return item, int(row.size)

    def run(self, items, consume):
        try:
            items = iter(items)
            cur, k = self._stage(0, next(items, None)), 0
            while cur is not None:
                _lib.ctx_wait(self.ctx, self.aux)       # landed: row k is there before its kernels start
                nxt = self._stage(k + 1, next(items, None))
                row, n_row = cur
                if row.expect is not None and row.expect != n_row:
                    raise Exception("%s: %s has %d points, its wavenumber grid %d" % (self.who, row.label, n_row, row.expect))
                consume(row, self.devs[k & 1], n_row)
                if nxt is not None:
                    _sync(self.ctx)                     # wait: the kernels on row k are over, its slot and the grids are free
                    self.grids.trim()
                cur, k = nxt, k + 1
        finally:
            try:
                _sync(self.ctx)                         # a kernel may still read a slot or a grid when a row failed,
                _sync(self.aux)                         # and an upload may still be in flight
            finally:
                for blk in self.pinned + self.devs:
                    if blk is not None:
                        blk.free()
                self.pinned, self.devs = [None, None], [None, None]
                self.grids.trim(0)


def _bins_and_abscissae(who, wvno_low, wvno_high, gauss_pts):
    """``(low, high, g)`` as contiguous float64: the bin edges (1-D, one length) and the Gauss abscissae (inside (0, 1))."""
    low, high, g = _lib.f64(wvno_low), _lib.f64(wvno_high), _lib.f64(gauss_pts)
    if g.ndim != 1 or g.size < 1:
        raise Exception("%s: gauss_pts must be a non-empty 1-D array" % who)
    if not np.all((g > 0.0) & (g < 1.0)):
        raise Exception("%s: the Gauss abscissae must lie strictly inside (0, 1)" % who)
    if low.ndim != 1 or low.shape != high.shape:
        raise Exception("%s: wvno_low and wvno_high must be 1-D arrays of one length, got %s and %s"
                        % (who, low.shape, high.shape))
    return low, high, g


@_lib.serialized
def compute_ck(cxs, og_wvno_grid, wvno_low, wvno_high, gauss_pts, _lds_cap=0, _return_stats=False):
    """Correlated-k coefficients ``(npoints, nbins, ngauss)`` of line-by-line cross sections: the bin loop of the
    reference's ``compute_ck_molecular`` (opacity_factory.py:1927-1955) for ``npoints`` P-T points.

    ``cxs``: one row of cross sections, or a sequence of rows (anything with ``len`` and ``[i]``: rows are taken one at a
    time).  ``og_wvno_grid``: the ascending wavenumbers of the rows -- one array for all of them, or a sequence with one
    array per row (rows may differ in length).  ``wvno_low``, ``wvno_high``: the edges of the ``nbins`` bins; a point
    belongs to a bin when ``low < wavenumber <= high``.  ``gauss_pts``: the abscissae, strictly inside (0, 1).

    Per bin, as the reference: values ``<= 0`` become ``1e-200``; the coefficients are ``np.interp(gauss_pts, x,
    np.sort(np.log(values)))`` with ``x = arange(n) / (n - 1.)``; a bin with fewer than two points is ``-200``.  The two
    logarithms behind an element are the device's: it differs from numpy's by at most ``8 * 2^-53 * max|ln|`` of them.
    A NaN inside a bin is a ``PicasoHipError`` that names the bin.

    Rows go one at a time through two pinned blocks and two device buffers (``_UploadRing``).  Row ``i + 1`` is read and
    copied into its pinned block on the host first; its transfer then runs on a second stream while the kernels of row ``i``
    run.  Only the transfer overlaps the kernels: the host-side read of the next row does not.

    ``_lds_cap`` (tests): segments longer than this take the HBM selection path (0: the default, 16 384 points).
    ``_return_stats``: also return ``(npoints, nbins, ngauss, 2)``, the clamped order statistics behind every element."""
    rows = _rows_of(cxs)
    npoints = len(rows)
    low, high, g = _bins_and_abscissae("compute_ck", wvno_low, wvno_high, gauss_pts)
    nbins, ngauss = int(low.size), int(g.size)
    shared = isinstance(og_wvno_grid, np.ndarray) and og_wvno_grid.ndim == 1
    if not shared:
        if not hasattr(og_wvno_grid, "__len__") or len(og_wvno_grid) == 0:
            raise Exception("compute_ck: og_wvno_grid must be one array or one array per row")
        if np.ndim(og_wvno_grid[0]) == 0:
            og_wvno_grid, shared = np.asarray(og_wvno_grid, dtype=float), True
        elif len(og_wvno_grid) != npoints:
            raise Exception("compute_ck: %d grids for %d rows: give one grid, or one per row" % (len(og_wvno_grid), npoints))
    if npoints == 0 or nbins == 0:
        k = np.zeros((npoints, nbins, ngauss))
        return (k, np.zeros((npoints, nbins, ngauss, 2))) if _return_stats else k

    segments = _Segments(low, high)

    ctx, aux = _lib.context(), _lib.aux_context()
    lib = _lib.load()
    d_k = DeviceArray((npoints, nbins, ngauss), ctx)
    d_stats = DeviceArray((npoints, nbins, ngauss, 2), ctx) if _return_stats else None
    per = nbins * ngauss * 8

    def grid_of(i):
        return og_wvno_grid if shared else og_wvno_grid[i]

    def bin_row(row, d_row, n_row):
        i = row.index
        lo, n, _ = segments.on(grid_of(i))
        _lib.check(lib.picaso_ck_from_xsec_dev(
            ctx, n_row, d_row.addr, nbins, lo.ctypes.data_as(_c_ll_p), n.ctypes.data_as(_c_ll_p), ngauss, _lib.ptr(g),
            int(_lds_cap), d_k.addr + i * per, d_stats.addr + 2 * i * per if _return_stats else None), ctx)

    try:
        _UploadRing(ctx, aux, "compute_ck").run(
            (_Row("row %d" % i, rows, i, int(np.size(grid_of(i)))) for i in range(npoints)), bin_row)
        k = d_k.to_host()
        return (k, d_stats.to_host()) if _return_stats else k
    finally:
        for blk in (d_k, d_stats):
            if blk is not None:
                blk.free()


class _RowFiles:
    """The rows of a cross-section directory, read when they are asked for."""

    def __init__(self, paths, load, announce=None):
        self.paths, self.load, self.announce = paths, load, announce

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        row = self.load(self.paths[i])
        if self.announce is not None:
            self.announce(i)
        return row


def _load_npy(path):
    with open(path, "rb") as fh:
        return np.load(fh)


def _load_fortran(path):
    return np.fromfile(path, dtype=float)


def _unsupported(who, what, why):
    raise NotImplementedError("%s: %s is not supported: %s" % (who, what, why))


class _Directory:
    """``grid1460.csv`` of a cross-section directory: its columns, one entry per line in file order, and what follows
    from them (``nc_p``: lines per temperature in increasing temperature; ``npres``, ``ntemp``: the unique counts)."""

    def __init__(self, who, og_directory):
        self.who, self.root = who, og_directory
        self.grid_file = grid_file = os.path.join(og_directory, "grid1460.csv")
        if not os.path.isfile(grid_file):
            raise Exception("%s: %s does not exist" % (who, grid_file))
        grid = np.atleast_1d(np.genfromtxt(grid_file, delimiter=",", names=True))
        need = ("pressure_bar", "temperature_K", "file_number", "number_wave_pts", "delta_wavenumber", "start_wavenumber")
        missing = [c for c in need if c not in (grid.dtype.names or ())]
        if missing:
            raise Exception("%s: %s has no column %s" % (who, grid_file, ", ".join(missing)))
        self.pres = np.asarray(grid["pressure_bar"], dtype=float)
        self.temp = temp = np.asarray(grid["temperature_K"], dtype=float)
        self.ifile = np.asarray(grid["file_number"]).astype(int)
        self.numw = np.asarray(grid["number_wave_pts"]).astype(int)
        self.delwn = np.asarray(grid["delta_wavenumber"], dtype=float)
        self.start = np.asarray(grid["start_wavenumber"], dtype=float)
        self.nc_p = np.array([float(np.sum(temp == t)) for t in np.unique(temp)])
        self.npres, self.ntemp = len(np.unique(self.pres)), len(np.unique(temp))
        self._grids = {}

    def row_files(self, molecule):
        """``(directory, file name pattern, loader)`` of the rows of one gas; the forms that are not read say so."""
        who, ifile = self.who, self.ifile
        if molecule in ALKALIS:
            _unsupported(who, "the alkali csv form (molecule %r)" % molecule,
                         "there is no sample of the reference's alkali files to pin the reading against")
        mol_dir = os.path.join(self.root, molecule)
        if "hdf5" in molecule or "h5" in molecule or os.path.exists(mol_dir + ".h5"):
            _unsupported(who, "the HDF5 / h5 input form (%s)" % mol_dir,
                         "there is no sample of these files to pin the reading against; give .npy or p_ rows")
        if os.path.exists(os.path.join(mol_dir, "readomni.fits")):
            _unsupported(who, "the FITS side-file readomni.fits", "reading it needs astropy; put number_wave_pts, "
                         "delta_wavenumber and start_wavenumber into grid1460.csv")
        if os.path.exists(os.path.join(mol_dir, "wavelengths.txt")):
            _unsupported(who, "the Lupu text form (wavelengths.txt)",
                         "there is no sample of these files to pin the reading against")
        first = int(ifile[0]) if ifile.size else 0
        if os.path.isfile(os.path.join(mol_dir, "p_%d" % first)):
            name, load = "p_%d", _load_fortran
        elif os.path.isfile(os.path.join(mol_dir, "%d.npy" % first)):
            name, load = "%d.npy", _load_npy
        else:
            raise Exception("%s: %s holds neither %d.npy (a numpy file) nor p_%d (unformatted float64) for "
                            "the first line of grid1460.csv" % (who, mol_dir, first, first))
        if np.any(ifile < 1) or np.any(ifile > ifile.size):
            raise Exception("%s: file_number must lie in [1, %d], the lines of %s" % (who, ifile.size, self.grid_file))
        return mol_dir, name, load

    def check_fits_table(self):
        if len(self.ifile) > self.npres * self.ntemp:
            raise Exception("%s: %d P-T points do not fit a table of %d pressures x %d temperatures"
                            % (self.who, len(self.ifile), self.npres, self.ntemp))

    def grid_of(self, file_number):
        """The wavenumbers of the rows ``file_number``, from csv line ``file_number - 1``: one array object per distinct
        (numw, delwn, start), so that what is found per grid is found once."""
        i = int(file_number)
        key = (int(self.numw[i - 1]), float(self.delwn[i - 1]), float(self.start[i - 1]))
        if key not in self._grids:
            self._grids[key] = uniform_grid(*key)
        return self._grids[key]


def _new_grid(who, wv_file_name, new_wno, new_dwno, min_max_wavelength, R):
    """``(wvno_low, wvno_high, new_wno, new_dwno)`` from whichever of the three ways the caller gave the new grid."""
    if wv_file_name is not None:
        return get_wvno_grid(wv_file_name)
    if new_wno is not None and new_dwno is not None:
        new_wno, new_dwno = np.asarray(new_wno, dtype=float), np.asarray(new_dwno, dtype=float)
        return 0.5 * (2 * new_wno - new_dwno), 0.5 * (2 * new_wno + new_dwno), new_wno, new_dwno
    if min_max_wavelength is not None and R is not None:
        lo_wl, hi_wl = sorted(min_max_wavelength)
        return get_wvno_grid(None, lo_wl, hi_wl, R)
    raise Exception("%s: give wv_file_name, or new_wno and new_dwno, or min_max_wavelength and R" % who)


def _table_datasets(d, new_wno, new_dwno, gi, wi, k_coeff_arr):
    """The eight datasets of a k-table file with the reference's descriptions (opacity_factory.py:1974-1983)."""
    return {
        "nc_p": (d.nc_p, "this defines the number of pressure points per temperature grid"),
        "pressures": (d.pres, "bars"),
        "temperatures": (d.temp, "Kelvin"),
        "wno": (new_wno, "cm**(-1)"),
        "delta_wno": (new_dwno, "cm**(-1)"),
        "gauss_pts": (gi, "gauss points created with double gauss method"),
        "gauss_wts": (wi, "gauss weights created with double gauss method"),
        "kcoeffs": (k_coeff_arr, "k coefficients on a pressure x temperature x wavenumber x gauss pts array"),
    }


def _write_table(h5py, filename, datasets, **file_attrs):
    """A k-table HDF5 file: ``datasets`` is ``{name: (value, description)}``; ``file_attrs`` become attributes of the file."""
    with h5py.File(filename, "w") as f:
        for key, (value, attribute) in datasets.items():
            f.create_dataset(key, data=value).attrs["description"] = attribute
        for key, value in file_attrs.items():
            f.attrs[key] = value


def _fill_table(d, k, nbins, ngauss):
    """``k`` (npoints, nbins, ngauss) in file order -> ``[ctp, ctt]``: ctp wraps at npres, ctt steps."""
    k_coeff_arr = np.zeros((d.npres, d.ntemp, nbins, ngauss))
    idx = np.arange(len(d.ifile))
    k_coeff_arr[idx % d.npres, idx // d.npres] = k
    return k_coeff_arr


@_lib.serialized
def compute_ck_molecular(molecule, og_directory, order=4, gfrac=0.95, alkali_dir=None, wv_file_name=None,
                         min_max_wavelength=None, R=None, new_wno=None, new_dwno=None, climate_filename=None, verbose=True):
    """Correlated-k table of one gas from a directory of line-by-line cross sections: the reference's function of this name
    (opacity_factory.py:1748-2008), same arguments and return value.  ``og_directory`` holds ``grid1460.csv`` (columns
    ``pressure_bar, temperature_K, file_number, number_wave_pts, delta_wavenumber, start_wavenumber``, read with numpy) and
    the directory ``molecule`` with one row per P-T point: ``<file_number>.npy`` (the reference's "python" type) or
    unformatted ``p_<file_number>`` (``np.fromfile``, its "fortran_binary" type; taken when both are there, as the
    reference does); a row's wavenumbers are ``arange(number_wave_pts) * delta_wavenumber + start_wavenumber`` of csv line
    ``file_number - 1``.  The new grid: ``wv_file_name`` (wavenumber, width), or ``new_wno`` and ``new_dwno``, or
    ``min_max_wavelength`` (micron) and ``R``.  The abscissae are ``g_w_2gauss(order, gfrac)``.

    Returns ``k_coeff_arr`` ``(npres, ntemp, nbins, 2 * order)``, ``ln kappa``.  The P-T loop runs in file order and fills
    ``[ctp, ctt]``: ``ctp`` counts up and wraps to 0, stepping ``ctt``, at ``npres``, the number of unique pressures.  The
    reference wraps at a hard-coded 20, which is ``npres`` on its own 1460-point grid.  ``nc_p`` is the number of csv
    lines per temperature in increasing temperature, as ``read_ck_tables`` counts them.

    ``climate_filename``: write the table as HDF5 instead (datasets ``nc_p, pressures, temperatures, wno, delta_wno,
    gauss_pts, gauss_wts, kcoeffs``, each with the reference's ``description`` attribute; ``read_ck_tables`` reads a
    directory of such ``<gas>_1460.hdf5`` files) and return None; needs h5py.

    Not supported, each a ``NotImplementedError``: the FITS side-file ``readomni.fits`` (needs astropy), the Lupu text
    rows and ``wavelengths.txt``, the alkali csv rows (``molecule`` in Na, K, Rb, Cs, Li) and the HDF5 / h5 inputs (no
    sample of these formats to pin the reading against)."""
    who = "compute_ck_molecular"
    h5py = optics._h5py() if climate_filename is not None else None       # before an hour of work, not after
    ngauss = 2 * int(order)
    d = _Directory(who, og_directory)
    mol_dir, name, load = d.row_files(molecule)
    gi, wi = optics.g_w_2gauss(order, gfrac)
    wvno_low, wvno_high, new_wno, new_dwno = _new_grid(who, wv_file_name, new_wno, new_dwno, min_max_wavelength, R)
    d.check_fits_table()
    ifile, pres, temp = d.ifile, d.pres, d.temp
    grids = [d.grid_of(i) for i in ifile]

    def announce(idx):                              # the reference's progress line, when the row is taken up
        print(ifile[idx], pres[idx], temp[idx])

    rows = _RowFiles([os.path.join(mol_dir, name % int(i)) for i in ifile], load, announce if verbose else None)
    k = compute_ck(rows, grids, wvno_low, wvno_high, gi)
    k_coeff_arr = _fill_table(d, k, len(wvno_low), ngauss)
    if climate_filename is None:
        return k_coeff_arr
    _write_table(h5py, climate_filename, _table_datasets(d, new_wno, new_dwno, gi, wi, k_coeff_arr))
    return None


# ---------------------------------------------------------------------------------------------------------------------
# premixed tables: the abundance-weighted sum of the gases' cross sections on the device, then the bin kernels
# ---------------------------------------------------------------------------------------------------------------------
def are_arrays_different(arr1, arr2):
    """The reference's test of this name (opacity_factory.py:1720-1745): another length, or not ``np.array_equal``."""
    if arr1 is arr2:
        return False
    return len(arr1) != len(arr2) or not np.array_equal(arr1, arr2)


def premix_abundances(chemistry, temperature_K, pressure_bar):
    """``(abunds, abunds_map)`` of a premixed table: the rows of a Visscher chemistry table that belong to the P-T points of
    ``grid1460.csv``, as the reference's ``compute_sum_molecular`` selects them (opacity_factory.py:1570-1584), its 1460
    generalised to ``N = len(temperature_K)``, the number of csv lines.

    ``chemistry``: a file for ``chemistry.read_visscher_2121``, or a dictionary of columns (``pressure``, ``temperature``,
    one per species).  A table of more than ``N`` rows keeps those whose temperature is one of ``temperature_K`` and whose
    pressure is ``< 10**3.5``, in table order; that must leave ``N`` rows.  ``pressure`` and ``temperature`` are then
    dropped, and the first column is ``index``, the rows' positions in the table: what pandas' ``reset_index()`` leaves
    in the reference's DataFrame.  A table of exactly ``N`` rows is taken as it stands, all columns included.  Fewer rows
    are an error.

    ``abunds``: float64 ``(N, ncolumns)``; ``abunds_map``: the column names.  The weight of a gas at csv line
    ``file_number`` is ``abunds[file_number - 1, abunds_map.index(gas)]`` (:1707)."""
    if isinstance(chemistry, dict):
        table = chemistry
    else:
        from .chemistry import read_visscher_2121
        table = read_visscher_2121(chemistry)
    temperature_K, pressure_bar = np.asarray(temperature_K, dtype=float), np.asarray(pressure_bar, dtype=float)
    if temperature_K.ndim != 1 or temperature_K.shape != pressure_bar.shape:
        raise Exception("premix_abundances: temperature_K and pressure_bar must be 1-D arrays of one length, got %s and %s"
                        % (temperature_K.shape, pressure_bar.shape))
    N = int(temperature_K.size)
    names = list(table.keys())
    cols = [np.asarray(table[k], dtype=float) for k in names]
    nrows = int(cols[0].size) if cols else 0
    if any(c.ndim != 1 or c.size != nrows for c in cols):
        raise Exception("premix_abundances: the columns of the chemistry table must be 1-D arrays of one length")
    if nrows < N:
        raise Exception("premix_abundances: the chemistry table has %d rows, fewer than the %d P-T points of grid1460.csv"
                        % (nrows, N))
    if nrows > N:
        for need in ("temperature", "pressure"):
            if need not in table:
                raise Exception("premix_abundances: the chemistry table has %d rows for %d P-T points and no column %r to "
                                "select them by" % (nrows, N, need))
        keep = np.isin(np.asarray(table["temperature"], dtype=float), np.unique(temperature_K)) \
            & (np.asarray(table["pressure"], dtype=float) < 10 ** 3.5)
        index = np.nonzero(keep)[0]
        if index.size != N:
            raise Exception("premix_abundances: the chemistry table has %d rows; the temperatures of grid1460.csv and "
                            "pressure < 10**3.5 select %d of them, grid1460.csv has %d lines" % (nrows, index.size, N))
        picked = [(k, c[index]) for k, c in zip(names, cols) if k not in ("pressure", "temperature")]
        names = ["index"] + [k for k, _ in picked]
        cols = [index.astype(float)] + [c for _, c in picked]
    return np.ascontiguousarray(np.column_stack(cols)), names


def _gas_weights(who, abunds, abunds_map, ck_molecules, ifile):
    """``(npoints, ngases)``: row ``file_number - 1`` of every gas's column, per csv line."""
    missing = [m for m in ck_molecules if m not in abunds_map]
    if missing:
        raise Exception("%s: the chemistry table has no column for %s" % (who, ", ".join(missing)))
    w = abunds[np.asarray(ifile) - 1][:, [abunds_map.index(m) for m in ck_molecules]]
    if not np.all(np.isfinite(w)):
        raise Exception("%s: the chemistry table holds an abundance that is not finite" % who)
    return w


class _Point:
    """What one weighted sum is made of: ``rows[m]`` (read when asked for), ``weights[m]``, ``grids[m]`` or None (every
    row lies on ``out_grid``, or -- ``out_grid`` None too -- all rows have one length)."""

    def __init__(self, who, rows, weights, grids=None, out_grid=None):
        if not hasattr(rows, "__len__") or not hasattr(rows, "__getitem__") or len(rows) < 1:
            raise Exception("%s: rows must be a non-empty sequence of rows" % who)
        self.rows, self.grids, self.out_grid = rows, grids, out_grid
        self.weights = np.asarray(weights, dtype=float)
        if self.weights.shape != (len(rows),):
            raise Exception("%s: %d rows need %d weights, got an array of shape %s"
                            % (who, len(rows), len(rows), self.weights.shape))
        if not np.all(np.isfinite(self.weights)):
            raise Exception("%s: the weights must be finite, got %s" % (who, self.weights))
        if grids is not None:
            if out_grid is None:
                raise Exception("%s: rows on grids of their own need out_grid, the grid of the sum" % who)
            if len(grids) != len(rows):
                raise Exception("%s: %d grids for %d rows: give None, or one per row" % (who, len(grids), len(rows)))


def _sum_points(who, npoints, point, consume, keep_last=False):
    """The weighted sums of ``npoints`` points, one after the other, each formed in HBM and handed to ``consume(i, d_acc)``
    there.  ``point(i)`` gives the ``_Point`` (asked for when its first row is staged).  The rows of all points travel
    through ONE upload ring: row ``k + 1`` is staged while ``picaso_xsec_axpy_dev`` adds row ``k``, across the points'
    boundaries too.  In HBM: the sum, the ring's two rows, and -- only for rows that are interpolated -- the ring's grid
    copies: the grid of the sum and the source grids, at most five in all.  ``keep_last``: return the last sum's
    DeviceArray (the caller frees it)."""
    ctx, aux, lib = _lib.context(), _lib.aux_context(), _lib.load()
    ring = _UploadRing(ctx, aux, who)
    d_acc = None
    differ = {}

    def flat():
        for i in range(npoints):
            p = point(i)
            for m in range(len(p.rows)):
                label = "row %d of point %d" % (m, i) if npoints > 1 else "row %d" % m
                yield _Row(label, p.rows, m, int(np.size(p.grids[m])) if p.grids is not None else None, (i, p))

    def interpolated(p, m):
        """does row m lie on a grid that differs from the grid of the sum (found once per pair of grid objects)"""
        if p.grids is None:
            return False
        key = (id(p.grids[m]), id(p.out_grid))
        hit = differ.get(key)
        if hit is None or hit[0] is not p.grids[m] or hit[1] is not p.out_grid:
            if len(differ) > 64:
                differ.clear()
            hit = differ[key] = (p.grids[m], p.out_grid, are_arrays_different(p.out_grid, p.grids[m]))
        return hit[2]

    def add_row(row, d_row, n_row):
        nonlocal d_acc
        m, (i, p) = row.index, row.tag
        if m == 0:
            n_out = int(np.size(p.out_grid)) if p.out_grid is not None else n_row
            if d_acc is None or d_acc.size != n_out:
                if d_acc is not None:
                    d_acc.free()
                d_acc = DeviceArray((n_out,), ctx)
        if interpolated(p, m):
            d_out = ring.grids.get(p.out_grid, "out_grid")[0]
            d_src, start, step = ring.grids.get(p.grids[m], "the grid of " + row.label)
            args = (n_row, d_src, d_out, start, step)
        else:
            if n_row != d_acc.size:
                raise Exception("%s: %s has %d points, the sum %d" % (who, row.label, n_row, d_acc.size))
            args = (n_row, None, None, 0.0, 0.0)
        _lib.check(lib.picaso_xsec_axpy_dev(ctx, d_acc.size, d_acc.addr, int(m == 0), float(p.weights[m]), d_row.addr, *args),
                   ctx)
        if m == len(p.rows) - 1:
            consume(i, d_acc)

    try:
        ring.run(flat(), add_row)
        if keep_last:
            kept, d_acc = d_acc, None
            return kept
        return None
    finally:
        if d_acc is not None:
            d_acc.free()


@_lib.serialized
def weighted_sum(rows, weights, grids=None, out_grid=None, out="host"):
    """``sum_m weights[m] * rows[m]`` formed on the device as the reference forms the mixture of a premixed table
    (opacity_factory.py:1617, 1707-1713): ``s = 0; for m: s += weights[m] * rows[m]``, the product and the sum as separate
    IEEE operations, so the result is numpy's bit for bit.

    ``rows``: a sequence of M rows (anything with ``len`` and ``[i]``; rows are taken one at a time).  ``weights``: M finite
    floats.  ``grids``: None -- every row lies on ``out_grid``, or, with ``out_grid`` None too, all rows have one length -- or
    one ascending wavenumber array per row; a row whose grid differs from ``out_grid`` (``are_arrays_different``: another
    length, or not ``np.array_equal``) is first interpolated onto it with ``np.interp``'s arithmetic (:1710-1711), on the
    device.  The grids are numpy's: they are uploaded, never recomputed.

    Row ``m + 1`` is staged (pinned block, transfer on a second stream) while row ``m`` is added.  Returns the sum as a numpy
    array, or with ``out="device"`` as a ``DeviceArray`` that the caller frees."""
    if out not in ("host", "device"):
        raise Exception("weighted_sum: out must be 'host' or 'device', got %r" % (out,))
    p = _Point("weighted_sum", rows, weights, grids, out_grid)
    d = _sum_points("weighted_sum", 1, lambda i: p, lambda i, d_acc: None, keep_last=True)
    if out == "device":
        return d
    try:
        return d.to_host()
    finally:
        d.free()


class _GasRows:
    """The rows of one P-T point, one per gas, read when they are asked for."""

    def __init__(self, paths, loads):
        self.paths, self.loads = paths, loads

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, m):
        return self.loads[m](self.paths[m])


@_lib.serialized
def compute_ck_of_sums(points, og_wvno_grid, wvno_low, wvno_high, gauss_pts, _lds_cap=0, announce=None):
    """``compute_ck`` of weighted sums that never leave the device: ``(npoints, nbins, ngauss)``.  ``points[i]`` is
    ``(rows, weights)``; the sum of its rows (``weighted_sum``) lies on ``og_wvno_grid[i]`` and goes straight from
    ``picaso_xsec_axpy_dev`` to ``picaso_ck_from_xsec_dev``.  ``announce(i)`` is called when point ``i`` is done."""
    npoints = len(points)
    low, high, g = _bins_and_abscissae("compute_ck_of_sums", wvno_low, wvno_high, gauss_pts)
    if len(og_wvno_grid) != npoints:
        raise Exception("compute_ck_of_sums: %d grids for %d points" % (len(og_wvno_grid), npoints))
    nbins, ngauss = int(low.size), int(g.size)
    if npoints == 0 or nbins == 0:
        return np.zeros((npoints, nbins, ngauss))
    segments = _Segments(low, high)
    ctx, lib = _lib.context(), _lib.load()
    d_k = DeviceArray((npoints, nbins, ngauss), ctx)
    per = nbins * ngauss * 8

    def bin_sum(i, d_acc):
        lo, n, n_grid = segments.on(og_wvno_grid[i])
        if n_grid != d_acc.size:
            raise Exception("compute_ck_of_sums: the rows of point %d have %d points, their wavenumber grid %d"
                            % (i, d_acc.size, n_grid))
        _lib.check(lib.picaso_ck_from_xsec_dev(ctx, d_acc.size, d_acc.addr, nbins, lo.ctypes.data_as(_c_ll_p),
                                               n.ctypes.data_as(_c_ll_p), ngauss, _lib.ptr(g), int(_lds_cap),
                                               d_k.addr + i * per, None), ctx)
        if announce is not None:
            announce(i)

    try:
        _sum_points("compute_ck_of_sums", npoints, lambda i: _Point("compute_ck_of_sums", *points[i]), bin_sum)
        return d_k.to_host()
    finally:
        d_k.free()


def _premix_setup(who, ck_molecules, og_directory, chemistry_file):
    """What both producers of the mixture read: the csv, every gas's row files, the abundances and the weights."""
    if isinstance(ck_molecules, str):
        ck_molecules = [ck_molecules]
    ck_molecules = list(ck_molecules)
    if not ck_molecules:
        raise Exception("%s: ck_molecules names no gas" % who)
    d = _Directory(who, og_directory)
    files = [d.row_files(m) for m in ck_molecules]
    abunds, abunds_map = premix_abundances(chemistry_file, d.temp, d.pres)
    weights = _gas_weights(who, abunds, abunds_map, ck_molecules, d.ifile)
    points = [(_GasRows([os.path.join(mol_dir, name % int(i)) for mol_dir, name, _ in files], [f[2] for f in files]), w)
              for i, w in zip(d.ifile, weights)]
    return ck_molecules, d, abunds, abunds_map, points


def _bytes(names):
    """Strings as an array of byte strings: what ``read_ck_tables`` decodes."""
    return np.array([str(x).encode("utf-8") for x in names], dtype="S")


def _chemistry_name(chemistry_file):
    return chemistry_file if isinstance(chemistry_file, str) else "a dictionary of columns"


@_lib.serialized
def compute_ck_premixed(ck_molecules, og_directory, chemistry_file, order=4, gfrac=0.95, wv_file_name=None,
                        min_max_wavelength=None, R=None, new_wno=None, new_dwno=None, climate_filename=None, verbose=True,
                        _lds_cap=0):
    """The premixed correlated-k table of a gas mixture at one chemistry, from a directory of line-by-line cross sections:
    the reference's ``compute_sum_molecular`` (opacity_factory.py:1530-1718) and the ``sum_<i>`` branch of its
    ``compute_ck_molecular`` (:1895-1898, 1916-1919, 1985-1998) in one pass.  Per line of ``grid1460.csv``, in file order,
    the rows ``<gas>/<file_number>.npy`` or ``<gas>/p_<file_number>`` of every gas of ``ck_molecules`` (in that order; the
    file forms and refusals of ``compute_ck_molecular``) are summed on the device with the weights of
    ``premix_abundances(chemistry_file, ...)``, and the sum is binned where it lies: it is neither copied back nor
    uploaded again.  The new grid and the abscissae are given as to ``compute_ck_molecular``.

    Returns ``k_coeff_arr`` ``(npres, ntemp, nbins, 2 * order)``, filled ``[ctp, ctt]`` as ``compute_ck_molecular`` fills
    it.  ``climate_filename``: write the premixed HDF5 file instead -- the eight datasets of ``compute_ck_molecular`` and
    ``abunds``, ``abunds_map``, ``ck_molecules`` with the reference's ``description`` attributes, strings as byte strings,
    and the file attribute ``chemistry_file`` -- which ``read_ck_tables`` and ``RetrieveCKs.from_files(...,
    method="preweighted")`` read; returns None; needs h5py."""
    who = "compute_ck_premixed"
    h5py = optics._h5py() if climate_filename is not None else None       # before an hour of work, not after
    ngauss = 2 * int(order)
    ck_molecules, d, abunds, abunds_map, points = _premix_setup(who, ck_molecules, og_directory, chemistry_file)
    gi, wi = optics.g_w_2gauss(order, gfrac)
    wvno_low, wvno_high, new_wno, new_dwno = _new_grid(who, wv_file_name, new_wno, new_dwno, min_max_wavelength, R)
    d.check_fits_table()

    def announce(idx):
        print(d.ifile[idx], d.pres[idx], d.temp[idx])

    k = compute_ck_of_sums(points, [d.grid_of(i) for i in d.ifile], wvno_low, wvno_high, gi, _lds_cap=_lds_cap,
                           announce=announce if verbose else None)
    k_coeff_arr = _fill_table(d, k, len(wvno_low), ngauss)
    if climate_filename is None:
        return k_coeff_arr
    ck_data = _table_datasets(d, new_wno, new_dwno, gi, wi, k_coeff_arr)
    ck_data["abunds"] = (abunds, "matrix of abundances in v/v units. Order of first axes of array is defined with abunds_map "
                                 "key and second as a function of P and T indices also included in abunds_map")
    ck_data["abunds_map"] = (_bytes(abunds_map), "array of strings that defines the order of abunds key")
    ck_data["ck_molecules"] = (_bytes(ck_molecules), "molecules included in the ck weighted table")
    _write_table(h5py, climate_filename, ck_data, chemistry_file=_chemistry_name(chemistry_file))
    return None


@_lib.serialized
def compute_sum_molecular(ck_molecules, og_directory, chemistry_file, output_dir, output_filename, wv_file_name=None,
                          alkali_dir=None, min_max_wavelength=None, R=None, new_wno=None, new_dwno=None, verbose=True):
    """The reference's function of this name (opacity_factory.py:1530-1718), same arguments, same file: the abundance-
    weighted sums of the gases' cross sections, one dataset ``sum_<file_number>`` per line of ``grid1460.csv``, behind the
    header datasets ``ck_molecules, pressure_bar, temperature_K, file_number, abunds, abunds_map`` and the file attribute
    ``chemistry_file``.  Every sum is formed by ``weighted_sum`` on the device and copied back.  The wavelength arguments
    are accepted and, as in the reference, not used: the sums stay on the line-by-line grid.  ``alkali_dir``: the alkali
    csv form is not read (``compute_ck_molecular``).  Needs h5py, and says so before any work starts.

    ``compute_ck_premixed`` makes the table itself without this file."""
    who = "compute_sum_molecular"
    h5py = optics._h5py()
    ck_molecules, d, abunds, abunds_map, points = _premix_setup(who, ck_molecules, og_directory, chemistry_file)
    with h5py.File(os.path.join(output_dir, output_filename), "w") as f:
        f.attrs["chemistry_file"] = _chemistry_name(chemistry_file)
        f.create_dataset("ck_molecules", data=_bytes(ck_molecules))
        f.create_dataset("pressure_bar", data=d.pres)
        f.create_dataset("temperature_K", data=d.temp)
        f.create_dataset("file_number", data=d.ifile)
        f.create_dataset("abunds", data=abunds)
        f.create_dataset("abunds_map", data=_bytes(abunds_map))
        for i, p, t, (rows, weights) in zip(d.ifile, d.pres, d.temp, points):
            f.create_dataset("sum_%d" % i, data=weighted_sum(rows, weights, out_grid=d.grid_of(i)))
            if verbose:
                print("completed", i, p, t)
    return None


# ---------------------------------------------------------------------------------------------------------------------
# the sqlite opacity database: its schema and readers (reference opacity_factory.py:578-739, 1262-1470)
# ---------------------------------------------------------------------------------------------------------------------
def adapt_array(arr):
    """A numpy array as the blob the reference stores: the bytes of ``np.save``."""
    buf = io.BytesIO()
    np.save(buf, arr)
    return sqlite3.Binary(buf.getvalue())


def convert_array(blob):
    return np.load(io.BytesIO(blob)).copy()


def open_local(db_f):
    """``(cursor, connection)`` of a database whose ``array`` columns travel as numpy arrays both ways."""
    conn = sqlite3.connect(db_f, detect_types=sqlite3.PARSE_DECLTYPES)
    sqlite3.register_adapter(np.ndarray, adapt_array)
    sqlite3.register_converter("array", convert_array)
    return conn.cursor(), conn


_SCHEMA = (("header", "id INTEGER PRIMARY KEY, pressure_unit VARCHAR, temperature_unit VARCHAR, wavenumber_grid array, "
                      "continuum_unit VARCHAR, molecular_unit VARCHAR"),
           ("molecular", "id INTEGER PRIMARY KEY, ptid INTEGER, molecule VARCHAR, pressure FLOAT, temperature FLOAT, "
                         "opacity array"),
           ("continuum", "id INTEGER PRIMARY KEY, molecule VARCHAR, temperature FLOAT, opacity array"))
_HEADER_INSERT = ("INSERT INTO header (pressure_unit, temperature_unit, wavenumber_grid, continuum_unit, molecular_unit) "
                  "values (?,?,?,?,?)")
_HEADER_UNITS = ("bar", "kelvin", "cm-1 amagat-2", "cm2/molecule")


def build_skeleton(db_f):
    """An empty database with the reference's three tables ``header``, ``molecular`` and ``continuum`` (:622-669); tables
    of these names that the file already holds are dropped."""
    cur, conn = open_local(db_f)
    for name, columns in _SCHEMA:
        cur.execute("DROP TABLE IF EXISTS %s" % name)
        cur.execute("CREATE TABLE %s (%s)" % (name, columns))
    conn.commit()
    conn.close()


def _insert_header(cur, wno_grid):
    cur.execute(_HEADER_INSERT, _HEADER_UNITS[:2] + (np.array(wno_grid),) + _HEADER_UNITS[2:])


def insert_wno_grid(wno_grid, cur, con):
    """Write the header row (the units and ``wno_grid``, cm-1), commit and close the connection, as the reference does."""
    _insert_header(cur, wno_grid)
    con.commit()
    con.close()


def create_grid_minR(min_wavelength, max_wavelength, minimum_R):
    """``(grid, step)``: wavenumbers in constant steps between the two wavelengths (micron); the step gives the resolution
    ``minimum_R`` at ``min_wavelength``, so every other point is resolved better (:692-710)."""
    dwvno = 1e4 / (min_wavelength ** 2) * (min_wavelength / minimum_R)
    return np.arange(1e4 / max_wavelength, 1e4 / min_wavelength, dwvno), dwvno


def continuum_avail(db_file):
    """``(molecules, temperatures)`` of the continuum table, each unique and sorted."""
    cur, conn = open_local(db_file)
    cur.execute("SELECT molecule FROM continuum")
    molecules = [str(m) for m in np.unique(cur.fetchall())]
    cur.execute("SELECT temperature FROM continuum")
    temperatures = list(np.unique(cur.fetchall()))
    conn.close()
    return molecules, temperatures


def molecular_avail(db_file):
    """``(molecules, pt_pairs)``: the gases of the molecular table and its ``(ptid, pressure, temperature)`` by ptid."""
    cur, conn = open_local(db_file)
    cur.execute("SELECT ptid, pressure, temperature FROM molecular")
    pt_pairs = sorted(set(cur.fetchall()), key=lambda x: x[0])
    cur.execute("SELECT molecule FROM molecular")
    molecules = [str(m) for m in np.unique(cur.fetchall())]
    conn.close()
    return molecules, pt_pairs


def find_nearest_1d(array, value):
    """Index of the entry of ``array`` nearest ``value``; among equal entries the last (:1281-1289)."""
    u, first, count = np.unique(array, return_index=True, return_counts=True)
    i = np.abs(u - value).argmin(axis=0)
    return first[i] + (count[i] - 1)


def _select_in(cur, table, columns, molecules, key, values):
    cur.execute("SELECT %s FROM %s WHERE molecule in (%s) AND %s in (%s)"
                % (columns, table, ", ".join("?" * len(molecules)), key, ", ".join("?" * len(values))),
                list(molecules) + list(values))
    return cur.fetchall()


def get_continuum(db_file, species, temperature):
    """``{species: {T: opacity}, 'wavenumber': grid}`` for the lists ``species`` and ``temperature``; every temperature
    is replaced by the nearest one of the table (:1290-1356)."""
    if not isinstance(temperature, list):
        raise Exception("Make Temperature a list, even if it is single valued")
    if not isinstance(species, list):
        raise Exception("Make Species Input a list, even if it is single valued")
    cur, conn = open_local(db_file)
    cur.execute("SELECT temperature FROM continuum")
    have = np.unique(cur.fetchall())
    nearest = [float(have[find_nearest_1d(have, t)]) for t in temperature]
    out = {s: {} for s in species}
    for mol, t, opacity in _select_in(cur, "continuum", "molecule,temperature,opacity", species, "temperature", nearest):
        out[mol][t] = opacity
    cur.execute("SELECT wavenumber_grid FROM header")
    out["wavenumber"] = cur.fetchone()[0]
    conn.close()
    return out


def get_molecular(db_file, species, temperature, pressure):
    """``{species: {T: {P: opacity}}, 'wavenumber': grid}``: ``temperature[i]`` and ``pressure[i]`` are a pair, replaced
    by the nearest pair of the table (plain distance in (P, T), :1358-1440)."""
    for name, v in (("temperature", temperature), ("pressure", pressure), ("Species", species)):
        if not isinstance(v, list):
            raise Exception("Make %s a list, even if it is single valued" % name)
    if len(temperature) != len(pressure):
        raise Exception("Temperature and Pressure must be the same size because these are treated as pairs. "
                        "t=[500,600], p=[1.0, 0.01] will grab [500,1.0 ] and [600,0.01]")
    cur, conn = open_local(db_file)
    cur.execute("SELECT ptid, pressure, temperature FROM molecular")
    pt_pairs = sorted(set(cur.fetchall()), key=lambda x: x[0])
    ids = [min(pt_pairs, key=lambda c: math.hypot(c[1] - p, c[2] - t))[0] for p, t in zip(pressure, temperature)]
    out = {s: {pt_pairs[i - 1][2]: {} for i in ids} for s in species}
    for mol, _, p, t, opacity in _select_in(cur, "molecular", "molecule,ptid,pressure,temperature,opacity", species,
                                            "ptid", ids):
        out[mol][t][p] = opacity
    cur.execute("SELECT wavenumber_grid FROM header")
    out["wavenumber"] = cur.fetchone()[0]
    conn.close()
    return out


def delete_molecule(mol, db_filename):
    """Delete every row of gas ``mol`` from the molecular table."""
    conn = sqlite3.connect(db_filename)
    try:
        conn.execute("DELETE from molecular where molecule = ?", (mol,))
        conn.commit()
    finally:
        conn.close()


def insert_hitran_cia(original_file, molname, new_db, new_wno):
    raise NotImplementedError("insert_hitran_cia: HITRAN's .cia reader is not supported: there is no sample of these "
                              "files to pin the reading against")


# ---------------------------------------------------------------------------------------------------------------------
# continuum rows: the host functions in the reference's operation order, and the device route
# ---------------------------------------------------------------------------------------------------------------------
def _refdata_file(name):
    ref = os.environ.get("picaso_refdata")
    if ref is None:
        raise Exception("%s is looked up under $picaso_refdata/opacities, which is not set; or pass the table as arrays"
                        % name)
    return os.path.join(ref, "opacities", name)


def read_overtone_table(fname=None):
    """``(wavenumber (n), temperatures (ncol), values (n, ncol))`` of ``H2H2_ov2_eq.tbl``: a header line ``wavenumber T1
    T2 ...``, then one line per wavenumber."""
    fname = fname if fname is not None else _refdata_file("H2H2_ov2_eq.tbl")
    with open(fname) as fh:
        temps = np.array([float(x) for x in fh.readline().split()[1:]])
        body = np.array([[float(x) for x in line.split()] for line in fh if line.strip()])
    return body[:, 0].copy(), temps, body[:, 1:].copy()


def read_h2minus_table(fname=None):
    """``(theta (n), wavelength in angstrom (ncol), values (n, ncol))`` of ``h2minus.csv`` (Bell 1980, table 1): five
    comment lines, a header ``theta,lambda1,...``, one line per theta."""
    fname = fname if fname is not None else _refdata_file("h2minus.csv")
    with open(fname) as fh:
        lines = [line.strip() for line in fh.readlines()[5:] if line.strip()]
    lam = np.array([float(x) for x in lines[0].split(",")[1:]])
    body = np.array([[float(x) for x in line.split(",")] for line in lines[1:]])
    return body[:, 0].copy(), lam, body[:, 1:].copy()


def _tables(overtone_table, h2minus_table):
    ov = tuple(np.asarray(x, dtype=float) for x in (overtone_table if overtone_table is not None else read_overtone_table()))
    bell = tuple(np.asarray(x, dtype=float) for x in (h2minus_table if h2minus_table is not None else read_h2minus_table()))
    return ov, bell


def _has_continuum_rows(db_f):
    conn = sqlite3.connect(db_f)
    try:
        return conn.execute("SELECT COUNT(*) FROM continuum").fetchone()[0] > 0
    except sqlite3.OperationalError:            # no such table
        return False
    finally:
        conn.close()


def get_original_data(original_file, colnames, new_db, overwrite=False):
    """``(og_opacity, temperatures, old_wno, molecules)`` of a CIA file (:228-274): a line ``nwno ntemp``, then per
    temperature a line with the temperature alone and ``nwno`` lines ``wavenumber log10(opacity) ...``, one column per name
    of ``colnames`` (``['wno', 'H2H2', ...]``).  As in the reference a line is a temperature when its second column is
    missing, and lines with any missing column are dropped from the data.  ``og_opacity``: ``{column: array}`` over the
    data lines.  Numbers are read with ``float``; the reference reads them with pandas, which gives the same bits for the
    decimal forms of these files.

    ``overwrite``: the reference's test is inverted (it raises when ``overwrite`` is True).  Here a ``new_db`` that already
    holds continuum rows raises unless ``overwrite=True``, which deletes them."""
    ncol = len(colnames)
    table = []
    with open(original_file) as fh:
        for line in fh:
            tok = line.split()
            if tok:
                table.append([float(x) for x in tok[:ncol]] + [np.nan] * (ncol - len(tok)))
    table = np.array(table, dtype=float).reshape(-1, ncol)
    temperatures = table[np.isnan(table[:, 1]), 0]
    data = table[~np.isnan(table).any(axis=1)]
    og_opacity = {c: data[:, k].copy() for k, c in enumerate(colnames)}
    _, first = np.unique(data[:, 0], return_index=True)
    old_wno = data[np.sort(first), 0]           # in order of appearance, as pandas' unique
    if os.path.exists(new_db) and _has_continuum_rows(new_db):
        if not overwrite:
            raise Exception("%s already holds continuum rows; overwrite=True deletes them first" % new_db)
        conn = sqlite3.connect(new_db)
        conn.execute("DELETE FROM continuum")
        conn.commit()
        conn.close()
    return og_opacity, temperatures, old_wno, list(colnames[1:])


def h2h2_overtone(t, wno, overtone_table=None):
    """``(opacity, loc, add)``: the H2-H2 band at 0.8 micron on the points ``wno[loc]`` inside the table, from the column
    nearest ``t``; ``add`` is False above the table's last temperature (:365-391).  cm-1 amagat-2."""
    wn, temps, values = overtone_table if overtone_table is not None else read_overtone_table()
    if t > max(temps):
        return np.nan, np.nan, False
    it = (np.abs(temps - t)).argmin()
    loc = np.where((wno >= wn.min()) & (wno <= wn.max()))
    return 10 ** (np.interp(wno[loc], wn, np.log10(values[:, it]), right=-33, left=-33)), loc, True


_LINSKY = dict(sig0=np.array([4162.043, 8274.650, 12017.753]), d1=np.array([1.2750e5, 1.32e6, 1.32e6]),
               d2=np.array([2760., 2760., 2760.]), d3=np.array([0.40, 0.40, 0.40]), a1=np.array([-7.661, -9.70, -11.32]),
               a2=np.array([0.5725, 0.5725, 0.5725]), b1=np.array([0.9376, 0.9376, 0.9376]),
               b2=np.array([0.5616, 0.5616, 0.5616]))       # Lenzuni et al. (1991), table 8


def _linsky_params(t, va=3):
    """``(w, d, a, b, aa)`` of fit_linsky at temperature ``t`` (:413-430)."""
    L, k = _LINSKY, va - 1
    w = L["sig0"][k]
    d = L["d3"][k] * np.sqrt(L["d1"][k] + L["d2"][k] * t)
    a = 10 ** (L["a1"][k] + L["a2"][k] * np.log10(t))
    b = 10 ** (L["b1"][k] + L["b2"][k] * np.log10(t))
    aa = 4.0 / 13.0 * a / d * np.exp(1.5 * d / b)
    return w, d, a, b, aa


def fit_linsky(t, wno, va=3):
    """H2-H2 opacity of Linsky (1969) and Lenzuni et al. (1991) for the points that hold the -33 placeholder (:393-440).
    The reference's branch for ``wno < w`` is always overwritten by its branch for ``wno < w + 1.5 d``; two are left."""
    w, d, a, b, aa = _linsky_params(t, va)
    kappa = aa * wno * np.exp(-(wno - w) / b)
    near = np.where(wno < w + 1.5 * d)
    kappa[near] = a * d * wno[near] / ((wno[near] - w) ** 2 + d * d)
    return kappa


def _bell_row(t, h2minus_table):
    """``(wno_bell, kappa_bell)``: Bell's wavenumbers and the row of the theta nearest ``5040 / t`` in cm4/dyn."""
    theta, lam, values = h2minus_table
    itheta = find_nearest_1d(theta, 5040.0 / t)
    return 1e8 / lam, (10 ** np.log10(values)[itheta, :]) * 1e-26


def get_h2minus(t, new_wno, h2minus_table=None):
    """H2- free-free opacity (Bell 1980, table 1) in cm4/dyn on ``new_wno``, 1e-33 outside the table (:442-479)."""
    wno_bell, kappa_bell = _bell_row(t, h2minus_table if h2minus_table is not None else read_h2minus_table())
    return np.interp(new_wno, wno_bell, kappa_bell, left=1e-33, right=1e-33)


_HBF_COEFF = np.array([152.519, 49.534, -118.858, 92.536, -34.194, 4.982])[::-1]       # John (1988)
_HBF_LAMBDA_0 = 1.6419


def get_hminusbf(wno):
    """H- bound-free cross section (John 1988) in cm2: 1e-33 at and beyond the edge at 1.6419 micron (:481-508)."""
    wave = 1e4 / wno
    on = np.where(wno > 1e4 / _HBF_LAMBDA_0)
    f, x = np.zeros(np.size(wave)), np.zeros(np.size(wave))
    result = np.zeros(np.size(wave)) + 1e-33
    x[on] = np.sqrt(1.0 / wave[on] - 1.0 / _HBF_LAMBDA_0)
    for c in _HBF_COEFF:
        f[on] = f[on] * x[on] + c
    result[on] = (wave[on] * x[on]) ** 3 * f[on] * 1e-18
    return result


_HFF = (   # Bell & Berrington (1987): A..F for wavelengths above 0.3645 micron, then for the rest
    ([0.e0, 2483.346, -3449.889, 2200.040, -696.271, 88.283], [0.e0, 285.827, -1158.382, 2427.719, -1841.400, 444.517],
     [0.e0, -2054.291, 8746.523, -13651.105, 8624.970, -1863.864], [0.e0, 2827.776, -11485.632, 16755.524, -10051.530, 2095.288],
     [0.e0, -1341.537, 5303.609, -7510.494, 4400.067, -901.788], [0.e0, 208.952, -812.939, 1132.738, -655.020, 132.985]),
    ([518.1021, 473.2636, -482.2089, 115.5291, 0.0, 0.0], [-734.8666, 1443.4137, -737.1616, 169.6374, 0.0, 0.0],
     [1021.1775, -1977.3395, 1096.8827, -245.649, 0.0, 0.0], [-479.0721, 922.3575, -521.1341, 114.243, 0.0, 0.0],
     [93.1373, -178.9275, 101.7963, -21.9972, 0.0, 0.0], [-6.4285, 12.3600, -7.0571, 1.5097, 0.0, 0.0]))


def _hff_powers(t):
    """``t_coeff**((i + 1) / 2)`` for i in 0..5, ``t_coeff = 5040 / t``: the weights of get_hminusff's six sums."""
    t_coeff = 5040.0 / t
    return [t_coeff ** ((i + 1) / 2.0) for i in range(6)]


def get_hminusff(t, wno):
    """H- free-free cross section (Bell & Berrington 1987) in cm5, with stimulated emission; 1e-60 below 800 K, wavelengths
    below 0.1823 micron taken there, zero past 20 micron (:510-573)."""
    wave = 1e4 / wno
    nwave = np.size(wave)
    if t < 800:
        return np.zeros(nwave) + 1e-60
    powers = _hff_powers(t)
    hj = np.zeros((6, nwave))
    longw, midw = np.where(wave > 0.3645), np.where(wave <= 0.3645)
    wave[np.where(wave < 0.1823)] = 0.1823
    for i in range(6):
        for sel, (A, B, C, D, E, F) in ((longw, _HFF[0]), (midw, _HFF[1])):
            v = wave[sel]
            hj[i, sel] = 1e-29 * (v * v * A[i] + B[i] + (C[i] + (D[i] + (E[i] + F[i] / v) / v) / v) / v)
    hm_cx = np.zeros(nwave)
    for i in range(6):
        hm_cx += powers[i] * hj[i, :]
    past20 = np.where(wave > 20.0)
    if np.size(past20) > 0:
        hm_cx[past20] = np.zeros(np.size(past20))
    return hm_cx * 1.380658e-16 * t


def medfilt(x, kernel_size):
    """``scipy.signal.medfilt`` of a 1-D array in numpy: the median of ``kernel_size`` (odd) neighbours, zeros beyond the
    ends."""
    x = np.asarray(x, dtype=float)
    h = int(kernel_size) // 2
    padded = np.concatenate((np.zeros(h), x, np.zeros(h)))
    out = np.empty(x.size)
    step = max(1, (1 << 24) // int(kernel_size))            # about 128 MB of windows at a time
    for lo in range(0, x.size, step):
        hi = min(x.size, lo + step)
        win = np.lib.stride_tricks.sliding_window_view(padded[lo:hi + 2 * h], 2 * h + 1)
        out[lo:hi] = np.partition(win, h, axis=1)[:, h]
    return out


def smoothing_window(new_wno):
    """The median filter's window: the odd number of points that spans 90 cm-1 at the grid's first step (:300-302)."""
    new_wno = np.asarray(new_wno)
    if new_wno.size < 2:
        raise Exception("the new wavenumber grid needs at least 2 points (the first step sets the smoothing window)")
    return int(np.ceil(90 / (new_wno[1] - new_wno[0])) // 2 * 2 + 1)


def _h2h2_row(t, bundle, new_wno, kernel_size, overtone_table, smooth=True):
    """The reference's patches of one interpolated H2H2 row (:313-331), in place."""
    h2h2, loc, add = h2h2_overtone(t, new_wno, overtone_table)
    if add:
        bundle[loc] = h2h2
    loc_33 = np.where((bundle == 1e-33) & (new_wno >= 1000))
    bundle[loc_33] = fit_linsky(t, new_wno[loc_33])
    if len(loc_33[0]) != 0 and max(new_wno[loc_33] < 12000) and smooth:
        loc_smooth = np.where((new_wno > 9950) & (new_wno < 11200))
        if len(loc_smooth[0]) != 0:
            bundle[loc_smooth] = medfilt(np.array(bundle[loc_smooth]), kernel_size)
    return bundle


def continuum_rows_numpy(og_log_opacity, temperatures, old_wno, molecules, new_wno, overtone_table=None, h2minus_table=None,
                         smooth=True):
    """The rows ``restructure_opacity`` writes, as one block ``(ntemp, nspecies, nwno)`` in the species order ``molecules
    + ['H2-', 'H-bf', 'H-ff']``, on the host in the reference's operation order (:300-359): bit for bit what the reference
    inserts.  ``og_log_opacity``: ``(ntemp, nmolecules, nold)`` log10 opacities on ``old_wno``, -33 where there is none.
    ``overtone_table``, ``h2minus_table``: the two data tables as ``read_overtone_table`` / ``read_h2minus_table`` return
    them; default: read from ``$picaso_refdata/opacities``.  ``smooth=False`` (tests): no median filter."""
    ov, bell = _tables(overtone_table, h2minus_table)
    og = np.asarray(og_log_opacity, dtype=float)
    temperatures, new_wno = np.asarray(temperatures, dtype=float), np.asarray(new_wno, dtype=float)
    old_wno, molecules = np.asarray(old_wno, dtype=float), list(molecules)
    if og.shape != (temperatures.size, len(molecules), old_wno.size):
        raise Exception("continuum_rows: og_log_opacity must be (ntemp, nmolecules, nold) = (%d, %d, %d), got %s"
                        % (temperatures.size, len(molecules), old_wno.size, og.shape))
    kernel_size = smoothing_window(new_wno)
    zero_bundle = np.zeros(len(new_wno)) + 1e-33
    out = np.empty((temperatures.size, len(molecules) + 3, new_wno.size))
    hminusbf = None
    for i, t in enumerate(temperatures):
        for k, m in enumerate(molecules):
            bundle = 10 ** (np.interp(new_wno, old_wno, og[i, k], right=-33, left=-33))
            if m == "H2H2":
                _h2h2_row(t, bundle, new_wno, kernel_size, ov, smooth)
            out[i, k] = bundle
        n = len(molecules)
        out[i, n] = zero_bundle if t < 600.0 else get_h2minus(t, new_wno, bell)
        if t < 800.0:
            out[i, n + 1], out[i, n + 2] = zero_bundle, zero_bundle * 1e-30
        else:
            if hminusbf is None:
                hminusbf = get_hminusbf(new_wno)
            out[i, n + 1], out[i, n + 2] = hminusbf, get_hminusff(t, new_wno)
    return out


def _continuum_params(temperatures, npar, ov, bell):
    """What the device reads per temperature: ``par (ntemp, npar)`` in the order of csrc/contfactory.hip's ContPar,
    ``ov_log (ntemp, nov)`` the log10 of the nearest overtone column, ``bell_kappa (ntemp, nbell)`` the nearest Bell row."""
    wn, ov_temps, ov_values = ov
    p33 = np.power(10.0, np.array([-33.0]))[0]
    zero = (np.zeros(1) + 1e-33)[0]
    par = np.zeros((len(temperatures), npar))
    ov_log = np.zeros((len(temperatures), wn.size))
    bell_kappa = np.zeros((len(temperatures), bell[1].size))
    ov_all = np.log10(ov_values)
    for i, t in enumerate(temperatures):
        add = not (t > max(ov_temps))
        if add:
            ov_log[i] = ov_all[:, (np.abs(ov_temps - t)).argmin()]
        w, d, a, b, aa = _linsky_params(t)
        hot = not (t < 800.0)
        if not (t < 600.0):
            bell_kappa[i] = _bell_row(t, bell)[1]
        par[i, :14] = (add, d, a, b, aa, w, w + 1.5 * d, t, not (t < 600.0), zero, hot, zero, hot,
                       zero * 1e-30 if t < 800.0 else 1e-60)
        if hot:
            par[i, 14:20] = _hff_powers(t)
        par[i, 20:24] = (p33, 1e4 / _HBF_LAMBDA_0, 1.0 / _HBF_LAMBDA_0, p33 == 1e-33)
    return par, ov_log, bell_kappa


def _ascending(a):
    return a.size < 2 or bool(np.all(a[1:] >= a[:-1]))


class _ContinuumDevice:
    """The inputs of ``picaso_continuum_rows_dev`` resident on the device; ``rows(t0, t1, d_out, d_work)`` enqueues the
    kernels of the temperatures ``[t0, t1)`` and returns at once."""

    def __init__(self, og_log_opacity, temperatures, old_wno, molecules, new_wno, overtone_table, h2minus_table, smooth,
                 lds_cap):
        who = "continuum_rows"
        ov, bell = _tables(overtone_table, h2minus_table)
        og = _lib.f64(og_log_opacity)
        self.temperatures = temperatures = _lib.f64(temperatures)
        old_wno, new_wno, self.molecules = _lib.f64(old_wno), _lib.f64(new_wno), list(molecules)
        if og.shape != (temperatures.size, len(self.molecules), old_wno.size) or og.size == 0:
            raise Exception("%s: og_log_opacity must be (ntemp, nmolecules, nold) = (%d, %d, %d), got %s"
                            % (who, temperatures.size, len(self.molecules), old_wno.size, og.shape))
        if new_wno.ndim != 1:
            raise Exception("%s: new_wno must be a 1-D array" % who)
        wno_bell = 1e8 / bell[1]
        for name, g in (("old_wno", old_wno), ("the overtone table's wavenumbers", ov[0]), ("Bell's wavenumbers", wno_bell)):
            if not _ascending(g):
                raise Exception("%s: %s must ascend on the device route; continuum_rows_numpy takes any order" % (who, name))
        self.window = smoothing_window(new_wno)
        region = np.where((new_wno > 9950) & (new_wno < 11200))[0]
        if region.size and region[-1] - region[0] + 1 != region.size:
            raise Exception("%s: the points of new_wno inside (9950, 11200) cm-1 must be neighbours on the device route; "
                            "continuum_rows_numpy takes any order" % who)
        if region.size and self.window < 1:
            raise Exception("%s: new_wno must ascend at its first step (the smoothing window is %d)" % (who, self.window))
        self.lo, self.n = (int(region[0]), int(region.size)) if region.size else (0, 0)
        self.window = max(self.window, 1)
        self.smooth, self.lds_cap = int(bool(smooth)), int(lds_cap)
        self.ntemp, self.nmol, self.nold, self.nwno = temperatures.size, len(self.molecules), old_wno.size, new_wno.size
        self.nsp = self.nmol + 3
        self.h2h2 = self.molecules.index("H2H2") if "H2H2" in self.molecules else -1
        self.ctx, self.lib = _lib.context(), _lib.load()
        self.npar = int(self.lib.picaso_continuum_npar())
        if self.npar != 24:
            raise Exception("%s: the library reads %d values per temperature, this module writes 24: rebuild it" % (who, self.npar))
        par, ov_log, bell_kappa = _continuum_params(temperatures, self.npar, ov, bell)
        self.nov, self.nbell = ov[0].size, wno_bell.size
        self.held = [DeviceArray.from_host(a, self.ctx) for a in (old_wno, og, new_wno, ov[0], ov_log, wno_bell, bell_kappa, par)]
        self.d_old, self.d_og, self.d_new, self.d_ovw, self.d_ovl, self.d_bw, self.d_bk, self.d_par = self.held

    def work(self, ntemp):
        return DeviceArray((ntemp * (self.n + 1),), self.ctx)

    def rows(self, t0, t1, d_out, d_work):
        _lib.check(self.lib.picaso_continuum_rows_dev(
            self.ctx, t1 - t0, self.nmol, self.h2h2, self.nold, self.d_old.addr, self.d_og.addr + 8 * t0 * self.nmol * self.nold,
            self.nwno, self.d_new.addr, self.nov, self.d_ovw.addr, self.d_ovl.addr + 8 * t0 * self.nov, self.nbell,
            self.d_bw.addr, self.d_bk.addr + 8 * t0 * self.nbell, self.d_par.addr + 8 * t0 * self.npar, self.lo, self.n,
            self.window, self.lds_cap, self.smooth, d_work.addr, d_out.addr), self.ctx)

    def free(self):
        try:
            _sync(self.ctx)
        finally:
            for blk in self.held:
                blk.free()
            self.held = []


_MAX_TEMPS_PER_CALL = 65535


@_lib.serialized
def continuum_rows(og_log_opacity, temperatures, old_wno, molecules, new_wno, overtone_table=None, h2minus_table=None,
                   out="host", smooth=True, _lds_cap=0):
    """``continuum_rows_numpy`` on the device (``picaso_continuum_rows_dev``, csrc/contfactory.hip): the same block
    ``(ntemp, nspecies, nwno)``, species ``molecules + ['H2-', 'H-bf', 'H-ff']``.  What depends on the temperature alone is
    formed here in numpy and uploaded; the per-point arithmetic runs in numpy's operation order without contraction.
    Against the host rows: H2-, H-ff, the constant rows and the Linsky points below ``w + 1.5 d`` are equal bit for bit;
    ``10**x`` is within 4 ulp; the Linsky points above and H-bf within 8 ulp; the smoothed region is
    the exact median of the device's own unsmoothed values.

    ``old_wno`` and the tables' wavenumbers must ascend, and the points of ``new_wno`` inside (9950, 11200) cm-1 must be
    neighbours.  ``out="device"``: a ``DeviceArray`` the caller frees.  ``smooth=False`` (tests): no median filter.
    ``_lds_cap`` (tests): windows longer than this take the radix-select path (0: the default, 8 192)."""
    if out not in ("host", "device"):
        raise Exception("continuum_rows: out must be 'host' or 'device', got %r" % (out,))
    dev = _ContinuumDevice(og_log_opacity, temperatures, old_wno, molecules, new_wno, overtone_table, h2minus_table, smooth,
                           _lds_cap)
    d_out = d_work = None
    try:
        d_out = DeviceArray((dev.ntemp, dev.nsp, dev.nwno), dev.ctx)
        d_work = dev.work(min(dev.ntemp, _MAX_TEMPS_PER_CALL))
        for t0 in range(0, dev.ntemp, _MAX_TEMPS_PER_CALL):
            t1 = min(dev.ntemp, t0 + _MAX_TEMPS_PER_CALL)
            dev.rows(t0, t1, d_out.row_range(t0, t1), d_work)
        if out == "device":
            _sync(dev.ctx)
            kept, d_out = d_out, None
            return kept
        return d_out.to_host()
    finally:
        dev.free()
        for blk in (d_out, d_work):
            if blk is not None:
                blk.free()


def _log_opacity_block(og_opacity, ntemp, molecules, nold):
    """``(ntemp, nmolecules, nold)`` from the columns of ``get_original_data``: temperature ``i`` owns the data lines
    ``[i nold, (i + 1) nold)`` (:310)."""
    block = np.empty((ntemp, len(molecules), nold))
    for k, m in enumerate(molecules):
        col = np.asarray(og_opacity[m], dtype=float)
        if col.size < ntemp * nold:
            raise Exception("restructure_opacity: column %s holds %d values, fewer than %d temperatures x %d wavenumbers"
                            % (m, col.size, ntemp, nold))
        block[:, k, :] = col[:ntemp * nold].reshape(ntemp, nold)
    return block


CONTINUUM_BUDGET_BYTES = 1 << 30


@_lib.serialized
def restructure_opacity(new_db, ntemp, temperatures, molecules, og_opacity, old_wno, new_wno, rows="device",
                        budget_bytes=None, overtone_table=None, h2minus_table=None):
    """Interpolate the CIA file's opacities onto ``new_wno``, add the other continuum sources and insert every row into
    the ``continuum`` table of ``new_db`` (the reference's function and arguments, :280-362; ``og_opacity``: the columns
    ``get_original_data`` returns).  Per temperature the rows go in as the reference inserts them: the molecules, then
    ``H2-``, ``H-bf``, ``H-ff``.

    ``rows="device"``: the rows are made by ``continuum_rows`` in chunks of temperatures of at most ``budget_bytes``
    (default 1 GiB; at least one temperature) each; two chunks are resident, and the copy back and the inserts of one
    overlap the kernels of the next.  ``rows="numpy"``: ``continuum_rows_numpy``, chunked the same way."""
    if rows not in ("device", "numpy"):
        raise Exception("restructure_opacity: rows must be 'device' or 'numpy', got %r" % (rows,))
    temperatures, new_wno = np.asarray(temperatures, dtype=float)[:ntemp], np.asarray(new_wno, dtype=float)
    molecules = list(molecules)
    block = _log_opacity_block(og_opacity, ntemp, molecules, len(old_wno))
    names = molecules + ["H2-", "H-bf", "H-ff"]
    budget = CONTINUUM_BUDGET_BYTES if budget_bytes is None else int(budget_bytes)
    per = max(1, min(budget // (8 * len(names) * max(1, new_wno.size)), _MAX_TEMPS_PER_CALL, max(1, ntemp)))
    chunks = [(t0, min(ntemp, t0 + per)) for t0 in range(0, ntemp, per)]
    cur, conn = open_local(new_db)

    def insert(t0, t1, host):
        for i in range(t0, t1):
            for k, name in enumerate(names):
                cur.execute("INSERT INTO continuum (molecule, temperature, opacity) values (?,?,?)",
                            (name, float(temperatures[i]), host[i - t0, k]))

    try:
        try:
            cur.execute("SELECT COUNT(*) FROM continuum")
        except sqlite3.OperationalError:
            raise Exception("restructure_opacity: %s has no continuum table; run build_skeleton first" % new_db) from None
        if rows == "numpy":
            for t0, t1 in chunks:
                insert(t0, t1, continuum_rows_numpy(block[t0:t1], temperatures[t0:t1], old_wno, molecules, new_wno,
                                                    overtone_table, h2minus_table))
        else:
            dev = _ContinuumDevice(block, temperatures, old_wno, molecules, new_wno, overtone_table, h2minus_table, True, 0)
            held = []
            try:
                shape = (per, len(names), new_wno.size)
                slots = []
                for _ in range(min(2, len(chunks))):
                    slots.append((DeviceArray(shape, dev.ctx), dev.work(per), PinnedArray(shape, dev.ctx)))
                    held.extend(slots[-1])
                waiting = None
                for c, (t0, t1) in enumerate(chunks):
                    d_out, d_work, pinned = slots[c & 1]
                    dev.rows(t0, t1, d_out, d_work)
                    mark = ctypes.c_void_p()
                    _lib.check(dev.lib.picaso_memcpy_d2h_async(dev.ctx, pinned.addr, d_out.addr,
                                                               8 * (t1 - t0) * len(names) * new_wno.size,
                                                               ctypes.byref(mark)), dev.ctx)
                    pinned._mark, pinned._mark_ctx = mark, dev.ctx
                    if waiting is not None:             # the rows of the chunk before, while this one's kernels run
                        insert(waiting[0], waiting[1], waiting[2].wait())
                    waiting = (t0, t1, pinned)
                if waiting is not None:
                    insert(waiting[0], waiting[1], waiting[2].wait())
            finally:
                dev.free()
                for blk in held:
                    blk.free()
        conn.commit()
    finally:
        conn.close()


def restruct_continuum(original_file, colnames, new_wno, new_db, overwrite=False, **kwargs):
    """The continuum part of an opacity database from a CIA file (the reference's function and arguments, :22-59):
    ``get_original_data`` then ``restructure_opacity`` (``kwargs`` go to it).  ``new_db`` must have the tables of
    ``build_skeleton``.

    ``overwrite``: the reference's test is inverted (it raises when ``overwrite`` is True and never deletes).  Here a
    ``new_db`` that already holds continuum rows raises unless ``overwrite=True``, which deletes them first."""
    og_opacity, temperatures, old_wno, molecules = get_original_data(original_file, colnames, new_db, overwrite=overwrite)
    restructure_opacity(new_db, len(temperatures), temperatures, molecules, og_opacity, old_wno, new_wno, **kwargs)


# ---------------------------------------------------------------------------------------------------------------------
# resampled molecular rows
# ---------------------------------------------------------------------------------------------------------------------
def resample_numpy(row, og_wvno_grid, points, insert_direct=False, min_wavelength=None, max_wavelength=None):
    """One molecular row as the reference forms it (:1023-1035), in numpy.  Resampled: ``np.interp`` onto ``points`` --
    every ``BINS``-th point of the hi-res grid, which is what the reference keeps of its interpolation onto the whole grid
    -- with fills and floor of 1e-100.  ``insert_direct``: the floor, then the points of the row whose wavelength lies
    strictly inside ``(min_wavelength, max_wavelength)``."""
    row = np.array(row, dtype=float)
    if insert_direct:
        keep = np.where((1e4 / og_wvno_grid > min_wavelength) & (1e4 / og_wvno_grid < max_wavelength))
        row[row < 1e-100] = 1e-100
        return row[keep]
    y = np.interp(points, og_wvno_grid, row, right=1e-100, left=1e-100)
    y[y < 1e-100] = 1e-100
    return y


@_lib.serialized
def insert_molecular_1460(molecule, min_wavelength, max_wavelength, og_directory, new_db, new_R=None, new_dwno=None,
                          old_R=1e6, old_dwno=0.0035, alkali_dir="alkalis", dir_kark_ch4=None, dir_optical_o3=None,
                          insert_direct=False):
    """Resample the cross sections of one gas onto a lower-resolution grid and insert them into the ``molecular`` table of
    ``new_db`` (the reference's function and arguments, :850-1055); returns the new wavenumber grid.  ``og_directory``
    holds ``grid1460.csv`` and the directory ``molecule`` with ``<file_number>.npy`` or ``p_<file_number>`` rows on
    uniform grids, as ``compute_ck_molecular`` reads them.

    ``new_R``: the hi-res grid is ``create_grid(min_wavelength, max_wavelength, old_R)`` and every ``int(old_R / new_R)``-th
    point of it is kept; ``new_dwno``: ``np.arange(1e4 / max_wavelength, 1e4 / min_wavelength, old_dwno)`` and every
    ``int(new_dwno / old_dwno)``-th point; both grids are built on the host as the reference builds them.  The reference
    interpolates every row onto the whole hi-res grid and then keeps the points; here only the kept points are uploaded,
    once, and ``picaso_xsec_resample_dev`` interpolates each row there (fills and floor 1e-100): the same values bit for
    bit.  The upload of the next row overlaps the kernel of the current one.  ``insert_direct``: the rows go in as they
    are, cut to the wavelength range, on the host.  Rows are inserted in file order; the header is written if the database
    has none.

    Not supported, each a ``NotImplementedError``: the alkali csv rows, the Lupu text rows, ``fort.*`` rows, the HDF5 / h5
    inputs, ``readomni.fits``, ``dir_kark_ch4`` and ``dir_optical_o3``."""
    who = "insert_molecular_1460"
    if dir_kark_ch4 is not None:
        _unsupported(who, "dir_kark_ch4 (Karkoschka methane)", "there is no sample of these files to pin the reading against")
    if dir_optical_o3 is not None:
        _unsupported(who, "dir_optical_o3 (optical ozone)", "there is no sample of these files to pin the reading against")
    if isinstance(new_R, (float, int)):
        from .justdoit import create_grid
        interp_wvno_grid, BINS = create_grid(min_wavelength, max_wavelength, old_R), int(old_R / new_R)
    elif isinstance(new_dwno, (float, int)):
        interp_wvno_grid, BINS = np.arange(1e4 / max_wavelength, 1e4 / min_wavelength, old_dwno), int(new_dwno / old_dwno)
    elif insert_direct:
        interp_wvno_grid, BINS = None, 1
    else:
        raise Exception("Need to either input a new constant R (new_R) or constant delta wno (new_dwno)")
    if BINS < 1:
        raise Exception("%s: the new resolution must not be finer than the old one (every %d-th point)" % (who, BINS))
    resample = interp_wvno_grid is not None and not insert_direct
    new_wvno_grid = np.ascontiguousarray(interp_wvno_grid[::BINS]) if resample else None
    d = _Directory(who, og_directory)
    mol_dir = os.path.join(og_directory, molecule)
    if glob.glob(os.path.join(mol_dir, "fort.*")) and not (glob.glob(os.path.join(mol_dir, "p_*"))
                                                           or glob.glob(os.path.join(mol_dir, "*npy*"))):
        _unsupported(who, "the fort.* text rows (%s)" % mol_dir, "there is no sample of these files to pin the reading against")
    mol_dir, name, load = d.row_files(molecule)
    paths = [os.path.join(mol_dir, name % int(i)) for i in d.ifile]
    cur, conn = open_local(new_db)

    def insert(k, y):
        cur.execute("INSERT INTO molecular (ptid, molecule, temperature, pressure,opacity) values (?,?,?,?,?)",
                    (int(d.ifile[k]), molecule, float(d.temp[k]), float(d.pres[k]), y))

    try:
        if not resample:
            for k, path in enumerate(paths):
                og = d.grid_of(d.ifile[k])
                row = load(path)
                if np.size(row) != og.size:
                    raise Exception("%s: row %s has %d points, its wavenumber grid %d" % (who, path, np.size(row), og.size))
                new_wvno_grid = og[np.where((1e4 / og > min_wavelength) & (1e4 / og < max_wavelength))]
                insert(k, resample_numpy(row, og, None, True, min_wavelength, max_wavelength))
        elif new_wvno_grid.size:
            ctx, aux, lib = _lib.context(), _lib.aux_context(), _lib.load()
            ring = _UploadRing(ctx, aux, who)
            d_points = DeviceArray.from_host(new_wvno_grid, ctx)
            d_out = DeviceArray((new_wvno_grid.size,), ctx)

            def resample_row(row, d_row, n_row):
                d_og, start, step = ring.grids.get(d.grid_of(d.ifile[row.index]), "the wavenumber grid of " + row.label)
                _lib.check(lib.picaso_xsec_resample_dev(ctx, new_wvno_grid.size, d_out.addr, d_row.addr, n_row, d_og,
                                                        d_points.addr, start, step, 1e-100, 1e-100, 1e-100), ctx)
                insert(row.index, d_out.to_host())

            try:
                files = _RowFiles(paths, load)
                ring.run((_Row("row %s" % path, files, k, d.grid_of(d.ifile[k]).size)
                          for k, path in enumerate(paths)), resample_row)
            finally:
                for blk in (d_points, d_out):
                    blk.free()
        else:
            for k in range(len(paths)):
                insert(k, np.zeros(0))
        conn.commit()
        cur.execute("SELECT pressure_unit from header")
        if len(cur.fetchall()) == 0:
            _insert_header(cur, new_wvno_grid)
            conn.commit()
    finally:
        conn.close()
    return new_wvno_grid
