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

A PREMIXED table (one ``ln kappa`` for a gas mixture at one chemistry, what ``opannection(method="preweighted")`` and the
climate solver run on) is the same binning of the abundance-weighted sum of the gases' rows, the reference's
``compute_sum_molecular`` (:1530-1718) followed by the ``sum_<i>`` branch of ``compute_ck_molecular``.
``jdi.compute_ck_premixed`` forms that sum in HBM (``picaso_xsec_axpy_dev``, csrc/xsecsum.hip: numpy's sum bit for bit) and
bins it there; ``jdi.weighted_sum`` is the array form of the sum, ``jdi.compute_sum_molecular`` writes the reference's
intermediate file, ``premix_abundances`` selects the abundances as the reference does.
"""
import ctypes
import os

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


class _UploadRing:
    """Two pinned blocks and two device buffers that rows of cross sections travel through one at a time, shared by
    ``compute_ck`` and the weighted sums.  ``stage(k, row, label)`` copies the row into the pinned block of slot ``k & 1`` on
    the host and enqueues its transfer on the second context's stream; it returns the row's length at once.  ``landed()``
    orders the first context's stream behind every transfer enqueued so far (the host does not block).  Before a slot is
    staged into again the caller has waited for the kernels that read it: that wait also says that the transfer out of its
    pinned block is over."""

    def __init__(self, ctx, aux, who):
        self.ctx, self.aux, self.who, self.lib = ctx, aux, who, _lib.load()
        self.pinned, self.devs = [None, None], [None, None]

    def stage(self, k, row, label):
        row = np.asarray(row, dtype=float)
        if row.ndim != 1 or row.size < 1:
            raise Exception("%s: %s must be a non-empty 1-D array, got shape %s" % (self.who, label, row.shape))
        s = k & 1
        if self.pinned[s] is None or self.pinned[s].shape != row.shape:
            for old in (self.pinned[s], self.devs[s]):
                if old is not None:
                    old.free()
            self.pinned[s], self.devs[s] = PinnedArray(row.shape, self.aux), DeviceArray(row.shape, self.ctx)
        self.pinned[s].array[:] = row
        _lib.check(self.lib.picaso_memcpy_h2d_async(self.aux, self.devs[s].addr, self.pinned[s].addr, 8 * row.size), self.aux)
        return int(row.size)

    def landed(self):
        _lib.ctx_wait(self.ctx, self.aux)

    def dev(self, k):
        return self.devs[k & 1]

    def free(self):
        try:
            _sync(self.aux)
        finally:
            for blk in self.pinned + self.devs:
                if blk is not None:
                    blk.free()
            self.pinned, self.devs = [None, None], [None, None]


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

    Rows go one at a time through two pinned blocks and two device buffers.  Row ``i + 1`` is read and copied into its
    pinned block on the host first; its transfer then runs on a second stream while the kernels of row ``i`` run.  Only the
    transfer overlaps the kernels: the call on a row waits for them, so the host-side read of the next row does not.

    ``_lds_cap`` (tests): segments longer than this take the HBM selection path (0: the default, 16 384 points).
    ``_return_stats``: also return ``(npoints, nbins, ngauss, 2)``, the clamped order statistics behind every element."""
    rows = _rows_of(cxs)
    npoints = len(rows)
    low, high = _lib.f64(wvno_low), _lib.f64(wvno_high)
    g = _lib.f64(gauss_pts)
    if g.ndim != 1 or g.size < 1:
        raise Exception("compute_ck: gauss_pts must be a non-empty 1-D array")
    if not np.all((g > 0.0) & (g < 1.0)):
        raise Exception("compute_ck: the Gauss abscissae must lie strictly inside (0, 1)")
    if low.ndim != 1 or low.shape != high.shape:
        raise Exception("compute_ck: wvno_low and wvno_high must be 1-D arrays of one length, got %s and %s"
                        % (low.shape, high.shape))
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
    ring = _UploadRing(ctx, aux, "compute_ck")
    try:
        n_next = ring.stage(0, rows[0], "row 0")
        for i in range(npoints):
            n_lbl = n_next
            ring.landed()                           # row i has landed before its kernels start
            if i + 1 < npoints:                     # its buffers are free: the call on row i - 1 has waited for its kernels
                n_next = ring.stage(i + 1, rows[i + 1], "row %d" % (i + 1))
            lo, n, n_grid = segments.on(og_wvno_grid if shared else og_wvno_grid[i])
            if n_grid != n_lbl:
                raise Exception("compute_ck: row %d has %d points, its wavenumber grid %d" % (i, n_lbl, n_grid))
            per = nbins * ngauss * 8
            _lib.check(lib.picaso_ck_from_xsec_dev(
                ctx, n_lbl, ring.dev(i).addr, nbins, lo.ctypes.data_as(_c_ll_p), n.ctypes.data_as(_c_ll_p), ngauss, _lib.ptr(g),
                int(_lds_cap), d_k.addr + i * per, d_stats.addr + 2 * i * per if _return_stats else None), ctx)
        k = d_k.to_host()
        return (k, d_stats.to_host()) if _return_stats else k
    finally:
        ring.free()                                 # waits for an upload that may still be in flight when a row fails
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
    with h5py.File(climate_filename, "w") as f:
        for key, (value, attribute) in _table_datasets(d, new_wno, new_dwno, gi, wi, k_coeff_arr).items():
            f.create_dataset(key, data=value).attrs["description"] = attribute
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
    boundaries too.  In HBM: the sum, the ring's two rows, and -- only for rows that are interpolated -- the grid of the sum
    and at most three source grids.  ``keep_last``: return the last sum's DeviceArray (the caller frees it)."""
    ctx, aux, lib = _lib.context(), _lib.aux_context(), _lib.load()
    ring = _UploadRing(ctx, aux, who)
    d_acc, d_out, d_src = None, None, {}            # d_out: (host grid, DeviceArray); d_src: id -> (host grid, DeviceArray)
    differ = {}

    def flat():
        for i in range(npoints):
            p = point(i)
            for m in range(len(p.rows)):
                yield i, m, p

    def label(item):
        return "row %d of point %d" % (item[1], item[0]) if npoints > 1 else "row %d" % item[1]

    def checked_grid(g, what):
        g = np.asarray(g, dtype=float)
        if g.ndim != 1 or g.size < 2 or not np.all(g[1:] >= g[:-1]):
            raise Exception("%s: %s must be an ascending 1-D array of at least 2 wavenumbers" % (who, what))
        return g

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

    try:
        items = flat()
        cur = next(items, None)
        n_next = ring.stage(0, cur[2].rows[cur[1]], label(cur)) if cur is not None else 0
        k = 0
        while cur is not None:
            i, m, p = cur
            n_row = n_next
            if k:
                _sync(ctx)                          # the kernel on row k - 1 is over: its slot and its grids are free
            while len(d_src) > 2:                   # room for this row's: at most three source grids at a time
                d_src.pop(next(iter(d_src)))[1].free()
            ring.landed()                           # row k has landed before its kernel starts
            nxt = next(items, None)
            if nxt is not None:
                n_next = ring.stage(k + 1, nxt[2].rows[nxt[1]], label(nxt))
            if m == 0:
                n_out = int(np.size(p.out_grid)) if p.out_grid is not None else n_row
                if d_acc is None or d_acc.size != n_out:
                    if d_acc is not None:
                        d_acc.free()
                    d_acc = DeviceArray((n_out,), ctx)
            if p.grids is not None and int(np.size(p.grids[m])) != n_row:
                raise Exception("%s: %s has %d points, its wavenumber grid %d" % (who, label(cur), n_row, np.size(p.grids[m])))
            if interpolated(p, m):
                if d_out is None or d_out[0] is not p.out_grid:
                    if d_out is not None:
                        d_out[1].free()
                    d_out = (p.out_grid, DeviceArray.from_host(checked_grid(p.out_grid, "out_grid"), ctx))
                g = p.grids[m]
                hit = d_src.get(id(g))
                if hit is None or hit[0] is not g:
                    hit = d_src[id(g)] = (g, DeviceArray.from_host(checked_grid(g, "the grid of " + label(cur)), ctx))
                step = (float(g[-1]) - float(g[0])) / (n_row - 1)
                args = (n_row, hit[1].addr, d_out[1].addr, float(g[0]), step if np.isfinite(step) and step > 0.0 else 0.0)
            else:
                if n_row != n_out:
                    raise Exception("%s: %s has %d points, the sum %d" % (who, label(cur), n_row, n_out))
                args = (n_row, None, None, 0.0, 0.0)
            _lib.check(lib.picaso_xsec_axpy_dev(ctx, n_out, d_acc.addr, int(m == 0), float(p.weights[m]), ring.dev(k).addr,
                                                *args), ctx)
            if m == len(p.rows) - 1:
                consume(i, d_acc)
            cur, k = nxt, k + 1
        if keep_last:
            kept, d_acc = d_acc, None
            return kept
        return None
    finally:
        try:
            _sync(ctx)                              # a kernel may still read what is freed below when a row fails
        finally:
            ring.free()
            for blk in [d_acc] + ([d_out[1]] if d_out else []) + [v[1] for v in d_src.values()]:
                if blk is not None:
                    blk.free()


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
    low, high, g = _lib.f64(wvno_low), _lib.f64(wvno_high), _lib.f64(gauss_pts)
    if g.ndim != 1 or g.size < 1 or not np.all((g > 0.0) & (g < 1.0)):
        raise Exception("compute_ck_of_sums: gauss_pts must be a non-empty 1-D array of abscissae strictly inside (0, 1)")
    if low.ndim != 1 or low.shape != high.shape:
        raise Exception("compute_ck_of_sums: wvno_low and wvno_high must be 1-D arrays of one length, got %s and %s"
                        % (low.shape, high.shape))
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
    with h5py.File(climate_filename, "w") as f:
        for key, (value, attribute) in ck_data.items():
            f.create_dataset(key, data=value).attrs["description"] = attribute
        f.attrs["chemistry_file"] = _chemistry_name(chemistry_file)
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
