"""Host side of the correlated-k factory (picaso_amd/opacity_factory.py): bins -> segments, the new wavenumber grid, the
argument errors, the parsing of a cross-section directory and the HDF5 output.  No GPU: the device call is replaced where a
test would reach it.  ``restate_ck`` is the numpy restatement of the reference's bin loop (opacity_factory.py:1927-1955)
that the GPU tests (test_ck_factory_gpu.py) compare against."""
import os
import sys

import numpy as np
import pytest

from picaso_amd import justdoit as jdi
from picaso_amd import opacity_factory as of
from picaso_amd import optics

HEADER = "pressure_bar,temperature_K,file_number,number_wave_pts,delta_wavenumber,start_wavenumber"


def restate_ck(row, og, wvno_low, wvno_high, gi):
    """The oracle: the k-coefficients of one row, bin by bin, in numpy (what reference opacity_factory.py:1927-1955
    computes).  A bin's points are those with ``low < og <= high``; non-positive values count as ``1e-200``; the sorted
    logarithms are read at ``gi`` on the abscissae ``j / (n - 1.)``; fewer than two points give ``-200``."""
    row, og = np.asarray(row, dtype=float), np.asarray(og, dtype=float)
    k = np.full((len(wvno_low), len(gi)), -200.0)
    with np.errstate(all="ignore"):
        for b, (lo, hi) in enumerate(zip(wvno_low, wvno_high)):
            seg = row[(og > lo) & (og <= hi)]
            if seg.size < 2:
                continue
            lnk = np.sort(np.log(np.where(seg <= 0.0, 1e-200, seg)))
            k[b] = np.interp(gi, np.arange(seg.size) / (seg.size - 1.), lnk)
    return k


def write_directory(root, molecule, rows, pres, temp, file_numbers, numw, delwn, start, form="npy"):
    """A cross-section directory as the reference expects it: grid1460.csv and one file per P-T point."""
    os.makedirs(os.path.join(root, molecule), exist_ok=True)
    with open(os.path.join(root, "grid1460.csv"), "w") as fh:
        fh.write(HEADER + "\n")
        for line in zip(pres, temp, file_numbers, numw, delwn, start):
            fh.write("%r,%r,%d,%d,%r,%r\n" % line)
    for i, row in zip(file_numbers, rows):
        if form == "npy":
            np.save(os.path.join(root, molecule, "%d.npy" % i), row)
        else:
            np.asarray(row, dtype=float).tofile(os.path.join(root, molecule, "p_%d" % i))


def mask_segments(og, low, high):
    lo, n = [], []
    for a, b in zip(low, high):
        idx = np.where((og > a) & (og <= b))[0]
        n.append(idx.size)
        lo.append(idx[0] if idx.size else None)
    return lo, np.array(n)


def check_segments(og, low, high):
    lo, n = of.ck_segments(og, low, high)
    assert lo.dtype == np.int64 and n.dtype == np.int64
    ref_lo, ref_n = mask_segments(og, low, high)
    assert np.array_equal(n, ref_n)
    for b in range(len(low)):
        assert 0 <= lo[b] and lo[b] + n[b] <= og.size
        if ref_n[b]:
            assert lo[b] == ref_lo[b]
    return lo, n


def test_ck_segments_match_the_mask_on_edges_overlaps_gaps_and_outside():
    og = np.array([10.0, 11.0, 12.0, 12.5, 13.0, 14.0, 15.0, 16.0, 17.0])
    low = np.array([10.0, 11.0, 12.0, 14.5, 30.0, 1.0, 12.4, 16.0, 9.0])
    high = np.array([12.0, 13.0, 14.0, 15.0, 40.0, 5.0, 12.6, 20.0, 100.0])
    lo, n = check_segments(og, low, high)
    assert (lo[0], n[0]) == (1, 2)              # 10.0 on the low edge is left out, 12.0 on the high edge is taken
    assert lo[1] < lo[0] + n[0]                 # bins 0 and 1 overlap
    assert n[4] == 0 and n[5] == 0              # wholly above and wholly below the grid
    assert n[6] == 1 and og[lo[6]] == 12.5      # a one-point bin
    assert lo[3] > lo[2] + n[2] - 1             # the gap between 14.0 and 14.5 belongs to nobody
    assert (lo[8], n[8]) == (0, 9)
    lo, n = of.ck_segments(og, np.array([13.0]), np.array([11.0]))          # low above high: empty, not negative
    assert n[0] == 0


def test_ck_segments_uniform_form_searches_the_numpy_grid():
    numw, delwn, start = 4001, 0.1, 100.0
    og = np.arange(numw) * delwn + start
    assert np.array_equal(of.uniform_grid(numw, delwn, start), og)
    rng = np.random.default_rng(3)
    picks = rng.integers(0, numw - 40, 30)
    low = np.concatenate((og[picks], og[picks] + 0.03))           # edges exactly on grid points, and between them
    high = np.concatenate((og[picks + 37], og[picks + 11]))
    lo, n = of.ck_segments_uniform(numw, delwn, start, low, high)
    ref_lo, ref_n = mask_segments(og, low, high)
    assert np.array_equal(n, ref_n) and np.array_equal(lo, np.array(ref_lo))
    assert np.all(n[:30] == 37) and np.all(lo[:30] == picks + 1)


def test_get_wvno_grid_in_both_modes(tmp_path):
    low, high, wno, dwno = of.get_wvno_grid(None, 1.0, 5.0, 50)
    ref = jdi.create_grid(1.0, 5.0, 50)
    d = list(np.diff(ref))
    d = np.array([d[0]] + d)
    assert np.array_equal(wno, ref) and np.array_equal(dwno, d)
    assert np.array_equal(low, 0.5 * (2 * ref - d)) and np.array_equal(high, 0.5 * (2 * ref + d))
    f = tmp_path / "wvno"
    w, dw = np.linspace(100.0, 900.0, 9), np.linspace(5.0, 45.0, 9)
    np.savetxt(f, np.column_stack((w, dw, np.zeros(9))))
    low, high, wno, dwno = of.get_wvno_grid(str(f))
    assert np.array_equal(wno, w) and np.array_equal(dwno, dw)
    assert np.array_equal(low, 0.5 * (2 * w - dw)) and np.array_equal(high, 0.5 * (2 * w + dw))


def test_argument_errors_are_raised_before_the_device_is_touched(tmp_path):
    og, row = np.arange(10.0), np.ones(10)
    low, high = np.array([0.5]), np.array([5.5])
    for g in ([0.0, 0.5], [0.5, 1.0], [np.nan], [-0.1], []):
        with pytest.raises(Exception, match="abscissae|gauss_pts"):
            of.compute_ck(row, og, low, high, g)
    with pytest.raises(Exception, match="one length"):
        of.compute_ck(row, og, low, np.array([1.0, 2.0]), [0.5])
    with pytest.raises(Exception, match="one grid, or one per row"):
        of.compute_ck([row, row, row], [og, og], low, high, [0.5])
    with pytest.raises(Exception, match="ascending"):
        of.ck_segments(og[::-1], low, high)
    with pytest.raises(Exception, match="1-D"):
        of.ck_segments(og.reshape(2, 5), low, high)
    assert of.compute_ck(row, og, np.zeros(0), np.zeros(0), [0.5]).shape == (1, 0, 1)
    assert jdi.compute_ck is of.compute_ck and jdi.compute_ck_molecular is of.compute_ck_molecular
    # compute_ck_molecular: what it does not read says so
    root = str(tmp_path)
    with pytest.raises(Exception, match="grid1460.csv"):
        of.compute_ck_molecular("H2O", root, new_wno=[1.0], new_dwno=[1.0], verbose=False)
    write_directory(root, "H2O", [row], [1.0], [100.0], [1], [10], [1.0], [0.0])
    with pytest.raises(NotImplementedError, match="alkali"):
        of.compute_ck_molecular("Na", root, new_wno=[1.0], new_dwno=[1.0], verbose=False)
    with pytest.raises(NotImplementedError, match="HDF5"):
        of.compute_ck_molecular("feh_000.hdf5", root, new_wno=[1.0], new_dwno=[1.0], verbose=False)
    with pytest.raises(Exception, match="wv_file_name, or new_wno and new_dwno, or min_max_wavelength and R"):
        of.compute_ck_molecular("H2O", root, verbose=False)
    with pytest.raises(Exception, match="holds neither 1.npy .* nor p_1"):
        os.makedirs(os.path.join(root, "CH4"))
        of.compute_ck_molecular("CH4", root, new_wno=[1.0], new_dwno=[1.0], verbose=False)
    open(os.path.join(root, "H2O", "readomni.fits"), "w").close()
    with pytest.raises(NotImplementedError, match="astropy"):
        of.compute_ck_molecular("H2O", root, new_wno=[1.0], new_dwno=[1.0], verbose=False)
    os.remove(os.path.join(root, "H2O", "readomni.fits"))
    open(os.path.join(root, "H2O", "wavelengths.txt"), "w").close()
    with pytest.raises(NotImplementedError, match="Lupu"):
        of.compute_ck_molecular("H2O", root, new_wno=[1.0], new_dwno=[1.0], verbose=False)


def fake_solver(calls):
    """Stands in for compute_ck: records what it was handed, returns the row's position in every element."""
    def fake(cxs, og_wvno_grid, wvno_low, wvno_high, gauss_pts):
        rows = [np.array(cxs[i]) for i in range(len(cxs))]
        calls.append(dict(rows=rows, grids=[np.array(g) for g in og_wvno_grid], low=np.array(wvno_low),
                          high=np.array(wvno_high), g=np.array(gauss_pts)))
        out = np.zeros((len(rows), len(wvno_low), len(gauss_pts)))
        for i in range(len(rows)):
            out[i] = i + 1
        return out
    return fake


def directory_case(root, form):
    """3 pressures x 2 temperatures in file order; file numbers are NOT the line order and every csv line has its own
    grid, so a row's grid must come from line ``file_number - 1``."""
    pres = [1e-3, 1e-1, 10.0, 1e-3, 1e-1, 10.0]
    temp = [500.0, 500.0, 500.0, 900.0, 900.0, 900.0]
    file_numbers = [3, 1, 2, 6, 5, 4]
    numw = [40, 41, 42, 43, 44, 45]
    delwn = [0.5, 0.25, 0.5, 0.25, 0.5, 0.25]
    start = [100.0, 101.0, 102.0, 103.0, 104.0, 105.0]
    rows = [np.full(numw[i - 1], float(i)) for i in file_numbers]
    write_directory(root, "H2O", rows, pres, temp, file_numbers, numw, delwn, start, form)
    return pres, temp, file_numbers, numw, delwn, start


@pytest.mark.parametrize("form", ["npy", "fortran"])
def test_directory_is_read_in_file_order_and_the_pressure_index_wraps_at_npres(tmp_path, monkeypatch, capsys, form):
    root = str(tmp_path)
    pres, temp, file_numbers, numw, delwn, start = directory_case(root, form)
    calls = []
    monkeypatch.setattr(of, "compute_ck", fake_solver(calls))
    new_wno, new_dwno = np.array([105.0, 110.0, 120.0]), np.array([4.0, 6.0, 10.0])
    k = of.compute_ck_molecular("H2O", root, order=2, gfrac=0.9, new_wno=new_wno, new_dwno=new_dwno)
    assert k.shape == (3, 2, 3, 4)
    (c,) = calls
    assert [r[0] for r in c["rows"]] == [float(i) for i in file_numbers]            # the files, in csv line order
    for r, g, i in zip(c["rows"], c["grids"], file_numbers):
        assert np.array_equal(g, np.arange(numw[i - 1]) * delwn[i - 1] + start[i - 1]) and r.size == g.size
    assert np.array_equal(c["low"], 0.5 * (2 * new_wno - new_dwno)) and np.array_equal(c["high"], 0.5 * (2 * new_wno + new_dwno))
    assert np.array_equal(c["g"], optics.g_w_2gauss(2, 0.9)[0])
    ctp = ctt = 0
    for idx in range(6):                                                             # the reference's counters
        assert np.all(k[ctp, ctt] == idx + 1)
        ctp += 1
        if ctp == 3:
            ctp, ctt = 0, ctt + 1
    printed = capsys.readouterr().out.split("\n")
    assert printed[0].split() == ["3", "0.001", "500.0"] and len([p for p in printed if p]) == 6
    # the other two ways to give the new grid
    f = tmp_path / "wv"
    np.savetxt(f, np.column_stack((new_wno, new_dwno)))
    of.compute_ck_molecular("H2O", root, wv_file_name=str(f), verbose=False)
    of.compute_ck_molecular("H2O", root, min_max_wavelength=[95.0, 80.0], R=20, verbose=False)
    assert np.array_equal(calls[1]["low"], c["low"])
    low, high = of.get_wvno_grid(None, 80.0, 95.0, 20)[:2]
    assert np.array_equal(calls[2]["low"], low) and np.array_equal(calls[2]["high"], high)
    assert not capsys.readouterr().out


class FakeH5py:
    """A dictionary-backed stand-in for the part of h5py the table writer and ``read_ck_tables`` use."""
    files = {}

    class Dataset:
        def __init__(self, data):
            self.data, self.attrs = np.array(data), {}

        def __getitem__(self, key):
            return self.data[key]

    class File:
        def __init__(self, path, mode="r"):
            if mode == "w":
                FakeH5py.files[path] = {}
                open(path, "w").close()
            self.sets = FakeH5py.files[path]

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def create_dataset(self, key, data=None):
            ds = self.sets[key] = FakeH5py.Dataset(data)
            return ds

        def __getitem__(self, key):
            return self.sets[key]


def test_climate_file_is_written_with_descriptions_and_read_back_by_read_ck_tables(tmp_path, monkeypatch):
    root = str(tmp_path)
    pres, temp = directory_case(root, "npy")[:2]
    monkeypatch.setattr(of, "compute_ck", fake_solver([]))
    monkeypatch.setattr(optics, "_h5py", lambda: FakeH5py)
    new_wno, new_dwno = np.array([105.0, 110.0, 120.0]), np.array([4.0, 6.0, 10.0])
    k = of.compute_ck_molecular("H2O", root, new_wno=new_wno, new_dwno=new_dwno, verbose=False)
    out_dir = tmp_path / "tables"
    out_dir.mkdir()
    path = str(out_dir / "H2O_1460.hdf5")
    assert of.compute_ck_molecular("H2O", root, new_wno=new_wno, new_dwno=new_dwno, climate_filename=path,
                                   verbose=False) is None
    sets = FakeH5py.files[path]
    assert sorted(sets) == sorted(["nc_p", "pressures", "temperatures", "wno", "delta_wno", "gauss_pts", "gauss_wts",
                                   "kcoeffs"])
    assert all(isinstance(ds.attrs["description"], str) and ds.attrs["description"] for ds in sets.values())
    assert sets["pressures"].attrs["description"] == "bars" and sets["wno"].attrs["description"] == "cm**(-1)"
    t = optics.read_ck_tables(str(out_dir), preload_gases=["H2O"])
    gi, wi = optics.g_w_2gauss(4, 0.95)
    assert np.array_equal(t["kappas"]["H2O"], k)
    assert np.array_equal(t["wno"], new_wno) and np.array_equal(t["delta_wno"], new_dwno)
    assert np.array_equal(t["gauss_pts"], gi) and np.array_equal(t["gauss_wts"], wi)
    assert np.array_equal(t["pressures"], np.unique(pres)) and np.array_equal(t["temps"], np.unique(temp))
    assert np.array_equal(t["nc_p"], [3, 3])


def test_climate_file_without_h5py_is_the_existing_error(tmp_path, monkeypatch):
    root = str(tmp_path)
    directory_case(root, "npy")
    calls = []
    monkeypatch.setattr(of, "compute_ck", fake_solver(calls))
    monkeypatch.setitem(sys.modules, "h5py", None)
    with pytest.raises(Exception, match="needs the h5py package"):
        of.compute_ck_molecular("H2O", root, new_wno=[105.0], new_dwno=[4.0], climate_filename=str(tmp_path / "x.hdf5"),
                                verbose=False)
    assert not calls                                # said before the work, not after it


def test_restatement_gives_the_reference_values_on_a_hand_case():
    """Three bins worked by hand: two points (the interpolation is a straight line between the two logarithms), one
    point and none."""
    og = np.array([1.0, 2.0, 3.0, 4.0])
    row = np.array([np.e, -1.0, np.e ** 3, 5.0])
    k = restate_ck(row, og, np.array([2.5, 3.5, 10.0, 0.0]), np.array([4.0, 4.0, 11.0, 2.0]), np.array([0.25, 0.5]))
    lo_, hi_ = np.log(5.0), 3.0
    assert np.allclose(k[0], lo_ + (hi_ - lo_) * np.array([0.25, 0.5]), rtol=1e-15)
    assert np.all(k[1] == -200.0) and np.all(k[2] == -200.0)
    assert np.allclose(k[3], np.log(1e-200) + (1.0 - np.log(1e-200)) * np.array([0.25, 0.5]), rtol=1e-15)
    assert row[1] == -1.0                           # the caller's row is left as it was
