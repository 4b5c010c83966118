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

    seg_cache = {}

    def segments(i):
        """``(lo, n, grid length)`` of row ``i``, found once per grid object"""
        og = og_wvno_grid if shared else og_wvno_grid[i]
        hit = seg_cache.get(id(og))
        if hit is None or hit[0] is not og:
            if len(seg_cache) > 8:
                seg_cache.clear()
            lo, n = ck_segments(og, low, high)
            hit = seg_cache[id(og)] = (og, np.ascontiguousarray(lo), np.ascontiguousarray(n), int(np.size(og)))
        return hit[1:]

    ctx, aux = _lib.context(), _lib.aux_context()
    lib = _lib.load()
    d_k = DeviceArray((npoints, nbins, ngauss), ctx)
    d_stats = DeviceArray((npoints, nbins, ngauss, 2), ctx) if _return_stats else None
    pinned, dev = [None, None], [None, None]

    def stage(i):
        """row ``i`` -> its pinned block -> its device buffer, on the second context's stream; returns at once"""
        row = np.asarray(rows[i], dtype=float)
        if row.ndim != 1 or row.size < 1:
            raise Exception("compute_ck: row %d must be a non-empty 1-D array, got shape %s" % (i, row.shape))
        s = i & 1
        if pinned[s] is None or pinned[s].shape != row.shape:
            for old in (pinned[s], dev[s]):
                if old is not None:
                    old.free()
            pinned[s], dev[s] = PinnedArray(row.shape, aux), DeviceArray(row.shape, ctx)
        pinned[s].array[:] = row
        _lib.check(lib.picaso_memcpy_h2d_async(aux, dev[s].addr, pinned[s].addr, 8 * row.size), aux)
        return int(row.size)

    try:
        n_next = stage(0)
        for i in range(npoints):
            n_lbl = n_next
            _lib.ctx_wait(ctx, aux)                 # row i has landed before its kernels start
            if i + 1 < npoints:
                n_next = stage(i + 1)               # its buffers are free: the call on row i - 1 has waited for its kernels
            lo, n, n_grid = segments(i)
            if n_grid != n_lbl:
                raise Exception("compute_ck: row %d has %d points, its wavenumber grid %d" % (i, n_lbl, n_grid))
            per = nbins * ngauss * 8
            _lib.check(lib.picaso_ck_from_xsec_dev(
                ctx, n_lbl, dev[i & 1].addr, nbins, lo.ctypes.data_as(_c_ll_p), n.ctypes.data_as(_c_ll_p), ngauss, _lib.ptr(g),
                int(_lds_cap), d_k.addr + i * per, d_stats.addr + 2 * i * per if _return_stats else None), ctx)
        k = d_k.to_host()
        return (k, d_stats.to_host()) if _return_stats else k
    finally:
        _sync(aux)                                  # an upload may still be in flight when a row fails
        for blk in pinned + dev + [d_k, d_stats]:
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


def _unsupported(what, why):
    raise NotImplementedError("compute_ck_molecular: %s is not supported: %s" % (what, why))


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
    h5py = optics._h5py() if climate_filename is not None else None       # before an hour of work, not after
    ngauss = 2 * int(order)
    grid_file = os.path.join(og_directory, "grid1460.csv")
    if not os.path.isfile(grid_file):
        raise Exception("compute_ck_molecular: %s does not exist" % grid_file)
    grid = np.atleast_1d(np.genfromtxt(grid_file, delimiter=",", names=True))
    need = ("pressure_bar", "temperature_K", "file_number", "number_wave_pts", "delta_wavenumber", "start_wavenumber")
    missing = [c for c in need if c not in (grid.dtype.names or ())]
    if missing:
        raise Exception("compute_ck_molecular: %s has no column %s" % (grid_file, ", ".join(missing)))
    pres, temp = np.asarray(grid["pressure_bar"], dtype=float), np.asarray(grid["temperature_K"], dtype=float)
    ifile = np.asarray(grid["file_number"]).astype(int)
    numw = np.asarray(grid["number_wave_pts"]).astype(int)
    delwn, start = np.asarray(grid["delta_wavenumber"], dtype=float), np.asarray(grid["start_wavenumber"], dtype=float)
    nc_p = np.array([float(np.sum(temp == t)) for t in np.unique(temp)])
    npres, ntemp = len(np.unique(pres)), len(np.unique(temp))

    if molecule in ALKALIS:
        _unsupported("the alkali csv form (molecule %r)" % molecule,
                     "there is no sample of the reference's alkali files to pin the reading against")
    mol_dir = os.path.join(og_directory, molecule)
    if "hdf5" in molecule or "h5" in molecule or os.path.exists(mol_dir + ".h5"):
        _unsupported("the HDF5 / h5 input form (%s)" % mol_dir,
                     "there is no sample of these files to pin the reading against; give .npy or p_ rows")
    if os.path.exists(os.path.join(mol_dir, "readomni.fits")):
        _unsupported("the FITS side-file readomni.fits", "reading it needs astropy; put number_wave_pts, "
                     "delta_wavenumber and start_wavenumber into grid1460.csv")
    if os.path.exists(os.path.join(mol_dir, "wavelengths.txt")):
        _unsupported("the Lupu text form (wavelengths.txt)", "there is no sample of these files to pin the reading against")
    first = int(ifile[0]) if ifile.size else 0
    if os.path.isfile(os.path.join(mol_dir, "p_%d" % first)):
        name, load = "p_%d", _load_fortran
    elif os.path.isfile(os.path.join(mol_dir, "%d.npy" % first)):
        name, load = "%d.npy", _load_npy
    else:
        raise Exception("compute_ck_molecular: %s holds neither %d.npy (a numpy file) nor p_%d (unformatted float64) for "
                        "the first line of grid1460.csv" % (mol_dir, first, first))
    if np.any(ifile < 1) or np.any(ifile > ifile.size):
        raise Exception("compute_ck_molecular: file_number must lie in [1, %d], the lines of %s" % (ifile.size, grid_file))

    gi, wi = optics.g_w_2gauss(order, gfrac)
    if wv_file_name is not None:
        wvno_low, wvno_high, new_wno, new_dwno = get_wvno_grid(wv_file_name)
    elif new_wno is not None and new_dwno is not None:
        new_wno, new_dwno = np.asarray(new_wno, dtype=float), np.asarray(new_dwno, dtype=float)
        wvno_low, wvno_high = 0.5 * (2 * new_wno - new_dwno), 0.5 * (2 * new_wno + new_dwno)
    elif min_max_wavelength is not None and R is not None:
        lo_wl, hi_wl = sorted(min_max_wavelength)
        wvno_low, wvno_high, new_wno, new_dwno = get_wvno_grid(None, lo_wl, hi_wl, R)
    else:
        raise Exception("compute_ck_molecular: give wv_file_name, or new_wno and new_dwno, or min_max_wavelength and R")
    if len(ifile) > npres * ntemp:
        raise Exception("compute_ck_molecular: %d P-T points do not fit a table of %d pressures x %d temperatures"
                        % (len(ifile), npres, ntemp))

    grids_by_key, grids = {}, []
    for i in ifile:                                 # one grid object per distinct (numw, delwn, start): found once
        key = (int(numw[i - 1]), float(delwn[i - 1]), float(start[i - 1]))
        if key not in grids_by_key:
            grids_by_key[key] = uniform_grid(*key)
        grids.append(grids_by_key[key])
    def announce(idx):                              # the reference's progress line, when the row is taken up
        print(ifile[idx], pres[idx], temp[idx])

    rows = _RowFiles([os.path.join(mol_dir, name % int(i)) for i in ifile], load, announce if verbose else None)
    k = compute_ck(rows, grids, wvno_low, wvno_high, gi)
    k_coeff_arr = np.zeros((npres, ntemp, len(wvno_low), ngauss))
    idx = np.arange(len(ifile))
    k_coeff_arr[idx % npres, idx // npres] = k      # ctp wraps at npres, ctt steps
    if climate_filename is None:
        return k_coeff_arr
    ck_data = {
        "nc_p": (nc_p, "this defines the number of pressure points per temperature grid"),
        "pressures": (pres, "bars"),
        "temperatures": (temp, "Kelvin"),
        "wno": (new_wno, "cm**(-1)"),
        "delta_wno": (new_dwno, "cm**(-1)"),
        "gauss_pts": (gi, "gauss points created with double gauss method"),
        "gauss_wts": (wi, "gauss weights created with double gauss method"),
        "kcoeffs": (k_coeff_arr, "k coefficients on a pressure x temperature x wavenumber x gauss pts array"),
    }
    with h5py.File(climate_filename, "w") as f:
        for key, (value, attribute) in ck_data.items():
            f.create_dataset(key, data=value).attrs["description"] = attribute
    return None
