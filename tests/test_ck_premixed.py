"""Host side of the premixed correlated-k tables (picaso_amd/opacity_factory.py: premix_abundances, compute_ck_premixed,
compute_sum_molecular, weighted_sum's arguments): the selection of the abundances against a pandas restatement of the
reference (opacity_factory.py:1570-1584), the reading of a directory of several gases, the files and the refusals.  No GPU:
the device call is replaced where a test would reach it (the GPU side: test_ck_premixed_gpu.py)."""
import os
import sys

import numpy as np
import pytest

from helpers import GOLDEN
from picaso_amd import justdoit as jdi
from picaso_amd import opacity_factory as of
from picaso_amd import optics
from test_ck_factory import write_directory

GASES = ["H2O", "CH4", "CO"]


@pytest.fixture(scope="module")
def table_2121():
    """The reference's ``sonora_2121grid_feh0.0_co0.55.txt`` as columns in file order, and the csv's two columns."""
    with np.load(os.path.join(GOLDEN, "chemistry.npz")) as z:
        table = {str(k): z["t2121/" + str(k)] for k in z["t2121/columns"]}
    with np.load(os.path.join(GOLDEN, "grid1460.npz")) as z:
        return table, z["temperature_K"], z["pressure_bar"]


def test_the_references_selection_keeps_the_1460_rows_of_the_2121_table_in_csv_order(table_2121):
    table, temp, pres = table_2121
    assert len(table["pressure"]) == 2121 and temp.shape == pres.shape == (1460,)
    abunds, names = of.premix_abundances(table, temp, pres)
    assert abunds.shape == (1460, len(table) - 1) and abunds.dtype == np.float64
    assert names == ["index"] + [k for k in table if k not in ("pressure", "temperature")]
    index = abunds[:, 0].astype(int)
    assert np.all(np.diff(index) > 0)                                   # table order
    assert np.array_equal(table["temperature"][index], temp)            # ... which is the csv's temperature order
    assert np.allclose(table["pressure"][index], pres, rtol=1e-3)       # half decades, 10**-5.523, against the csv's 3e-06
    out = np.setdiff1d(np.arange(2121), index)                          # every row left out fails one of the two tests
    assert np.all((table["pressure"][out] >= 10 ** 3.5) | ~np.isin(table["temperature"][out], temp))
    for gas in ("H2O", "CH4", "e-"):
        assert np.array_equal(abunds[:, names.index(gas)], table[gas][index])
    w = of._gas_weights("t", abunds, names, ["CH4", "H2O"], np.array([1460, 1, 731]))
    assert np.array_equal(w, [[table[g][index[i]] for g in ("CH4", "H2O")] for i in (1459, 0, 730)])


def test_abunds_and_abunds_map_equal_the_references_dataframe(table_2121):
    """Reference lines 1570-1584 restated with pandas on the same table: what ``f.create_dataset('abunds',
    data=chem_grid)`` and ``list(chem_grid.keys())`` hold, the ``index`` column of ``reset_index()`` included."""
    pd = pytest.importorskip("pandas")
    table, temp, pres = table_2121
    chem_grid = pd.DataFrame(table)
    s1460 = pd.DataFrame({"temperature_K": [repr(float(t)) for t in temp]}, dtype=str)
    assert chem_grid.shape[0] > 1460
    chem_grid = chem_grid.loc[chem_grid["temperature"].isin(s1460["temperature_K"].astype(float).unique())] \
        .loc[chem_grid["pressure"] < 10 ** 3.5].reset_index()
    assert chem_grid.shape[0] == 1460, "chem grid is still not 1460 shape"
    chem_grid = chem_grid.drop("pressure", axis=1)
    chem_grid = chem_grid.drop("temperature", axis=1)
    abunds, names = of.premix_abundances(table, temp, pres)
    assert names == list(chem_grid.keys())
    want = np.asarray(chem_grid, dtype=float)
    assert abunds.shape == want.shape and np.array_equal(abunds.view(np.uint64), want.view(np.uint64))
    for i, gas in ((0, "H2O"), (1459, "NH3"), (700, "CO")):             # weight = chem_grid.loc[i - 1, molecule]
        assert abunds[i, names.index(gas)] == chem_grid.loc[i, gas]


def small_table(nrows=6):
    rng = np.random.default_rng(8)
    return {"temperature": np.repeat([500.0, 900.0], 3)[:nrows], "pressure": np.tile([1e-3, 1e-1, 10.0], 2)[:nrows],
            "H2O": rng.uniform(1e-5, 1e-3, nrows), "CH4": rng.uniform(1e-7, 1e-4, nrows), "CO": rng.uniform(1e-6, 1e-4, nrows)}


def test_exactly_n_rows_are_taken_as_they_stand_and_the_errors():
    t = small_table()
    abunds, names = of.premix_abundances(t, t["temperature"], t["pressure"])
    assert names == list(t) and np.array_equal(abunds, np.column_stack([t[k] for k in t]))      # pressure, temperature kept
    # more rows: selected by temperature and by pressure < 10**3.5, in table order
    big = {k: np.concatenate((v[:2], [7.0], v[2:], [9.0])) for k, v in t.items()}
    big["temperature"][2], big["pressure"][2] = 700.0, 1.0            # a temperature the csv does not have
    big["temperature"][-1], big["pressure"][-1] = 900.0, 10 ** 3.5    # a pressure that is not < 10**3.5
    abunds, names = of.premix_abundances(big, t["temperature"], t["pressure"])
    assert names == ["index", "H2O", "CH4", "CO"]
    assert np.array_equal(abunds[:, 0], [0, 1, 3, 4, 5, 6]) and np.array_equal(abunds[:, 1], t["H2O"])
    with pytest.raises(Exception, match="8 rows.*select 5 of them.*6 lines"):
        big["pressure"][0] = 1e4
        of.premix_abundances(big, t["temperature"], t["pressure"])
    with pytest.raises(Exception, match="5 rows, fewer than the 6"):
        of.premix_abundances({k: v[:5] for k, v in t.items()}, t["temperature"], t["pressure"])
    with pytest.raises(Exception, match="no column 'temperature'"):
        of.premix_abundances({"H2O": np.ones(9)}, t["temperature"], t["pressure"])
    with pytest.raises(Exception, match="no column for NH3, Q"):
        of._gas_weights("t", abunds, names, ["H2O", "NH3", "Q"], np.arange(1, 7))
    with pytest.raises(Exception, match="not finite"):
        of._gas_weights("t", np.full((6, 1), np.nan), ["H2O"], ["H2O"], np.arange(1, 7))


def mixture_directory(root, forms=("npy", "fortran", "npy")):
    """3 pressures x 2 temperatures; file numbers are NOT the line order; every gas has its own file form; a row's values
    name its gas and its file: ``100 * gas + file_number``."""
    pres = [1e-3, 1e-1, 10.0, 1e-3, 1e-1, 10.0]
    temp = [500.0, 500.0, 500.0, 900.0, 900.0, 900.0]
    file_numbers = [3, 1, 2, 6, 5, 4]
    numw = [40, 41, 42, 43, 44, 45]
    delwn = [0.5, 0.25, 0.5, 0.25, 0.5, 0.25]
    start = [100.0, 101.0, 102.0, 103.0, 104.0, 105.0]
    for g, (gas, form) in enumerate(zip(GASES, forms)):
        rows = [np.full(numw[i - 1], 100.0 * g + i) for i in file_numbers]
        write_directory(root, gas, rows, pres, temp, file_numbers, numw, delwn, start, form)
    return pres, temp, file_numbers, numw, delwn, start


def fake_device(calls):
    """Stands in for compute_ck_of_sums: reads every row it is handed, returns the point's position in every element."""
    def fake(points, og_wvno_grid, wvno_low, wvno_high, gauss_pts, _lds_cap=0, announce=None):
        calls.append(dict(rows=[[np.array(rows[m]) for m in range(len(rows))] for rows, _ in points],
                          weights=[np.array(w) for _, w in points], grids=[np.array(g) for g in og_wvno_grid],
                          low=np.array(wvno_low), high=np.array(wvno_high), g=np.array(gauss_pts), cap=_lds_cap))
        out = np.zeros((len(points), len(wvno_low), len(gauss_pts)))
        for i in range(len(points)):
            out[i] = i + 1
            if announce is not None:
                announce(i)
        return out
    return fake


def test_directory_of_gases_is_read_in_file_order_with_the_weights_of_its_lines(tmp_path, monkeypatch, capsys):
    root = str(tmp_path)
    pres, temp, file_numbers, numw, delwn, start = mixture_directory(root)
    chem = small_table()
    calls = []
    monkeypatch.setattr(of, "compute_ck_of_sums", fake_device(calls))
    new_wno, new_dwno = np.array([105.0, 110.0, 120.0]), np.array([4.0, 6.0, 10.0])
    order = ["CO", "H2O", "CH4"]
    k = of.compute_ck_premixed(order, root, chem, order=2, gfrac=0.9, new_wno=new_wno, new_dwno=new_dwno)
    assert k.shape == (3, 2, 3, 4)
    (c,) = calls
    for rows, w, grid, i in zip(c["rows"], c["weights"], c["grids"], file_numbers):
        assert [r[0] for r in rows] == [100.0 * GASES.index(g) + i for g in order]      # ck_molecules' order, csv line order
        assert all(r.size == numw[i - 1] for r in rows)
        assert np.array_equal(grid, np.arange(numw[i - 1]) * delwn[i - 1] + start[i - 1])
        assert np.array_equal(w, [chem[g][i - 1] for g in order])                       # row file_number - 1 of the column
    assert np.array_equal(c["low"], 0.5 * (2 * new_wno - new_dwno)) and np.array_equal(c["g"], optics.g_w_2gauss(2, 0.9)[0])
    ctp = ctt = 0
    for idx in range(6):
        assert np.all(k[ctp, ctt] == idx + 1)
        ctp += 1
        if ctp == 3:
            ctp, ctt = 0, ctt + 1
    printed = [p for p in capsys.readouterr().out.split("\n") if p]
    assert printed[0].split() == ["3", "0.001", "500.0"] and len(printed) == 6
    of.compute_ck_premixed("H2O", root, chem, min_max_wavelength=[95.0, 80.0], R=20, verbose=False, _lds_cap=128)
    low, high = of.get_wvno_grid(None, 80.0, 95.0, 20)[:2]
    assert np.array_equal(calls[1]["low"], low) and np.array_equal(calls[1]["high"], high) and calls[1]["cap"] == 128
    assert [len(r) for r in calls[1]["rows"]] == [1] * 6 and not capsys.readouterr().out


def test_premixed_file_is_written_and_read_back_by_read_ck_tables(tmp_path, monkeypatch, h5py):
    root = str(tmp_path / "xsec")
    pres, temp = mixture_directory(root)[:2]
    chem = small_table()
    monkeypatch.setattr(of, "compute_ck_of_sums", fake_device([]))
    new_wno, new_dwno = np.array([105.0, 110.0, 120.0]), np.array([4.0, 6.0, 10.0])
    k = of.compute_ck_premixed(GASES, root, chem, new_wno=new_wno, new_dwno=new_dwno, verbose=False)
    path = str(tmp_path / "premixed_feh+000_co_100.hdf5")
    assert of.compute_ck_premixed(GASES, root, chem, new_wno=new_wno, new_dwno=new_dwno, climate_filename=path,
                                  verbose=False) is None
    with h5py.File(path, "r") as f:
        assert sorted(f.keys()) == sorted(["nc_p", "pressures", "temperatures", "wno", "delta_wno", "gauss_pts", "gauss_wts",
                                           "kcoeffs", "abunds", "abunds_map", "ck_molecules"])
        assert np.array_equal(f["nc_p"][:], [3.0, 3.0])
        assert all(isinstance(x, bytes) for x in f["abunds_map"][:]) and all(isinstance(x, bytes) for x in f["ck_molecules"][:])
    t = optics.read_ck_tables(path)
    gi, wi = optics.g_w_2gauss(4, 0.95)
    assert np.array_equal(t["kappa"], k) and t["molecules"] == GASES
    assert t["abunds_map"] == list(chem) and np.array_equal(t["abunds"], np.column_stack([chem[c] for c in chem]))
    assert np.array_equal(t["wno"], new_wno) and np.array_equal(t["delta_wno"], new_dwno)
    assert np.array_equal(t["gauss_pts"], gi) and np.array_equal(t["gauss_wts"], wi)
    assert np.array_equal(t["pressures"], np.unique(pres)) and np.array_equal(t["temps"], np.unique(temp))
    assert np.array_equal(t["nc_p"], [3, 3])
    full = {key: t["abunds"][:, i] for i, key in enumerate(t["abunds_map"])}       # what RetrieveCKs.from_files keeps
    assert np.array_equal(full["CH4"], chem["CH4"])


def test_descriptions_and_the_chemistry_file_attribute(tmp_path, monkeypatch):
    """The attributes, which the stand-in's files do not keep: seen on a recording h5py."""
    seen = {}

    class Recorder:
        class File:
            def __init__(self, path, mode="r"):
                self.attrs = seen.setdefault("file", {})

            def __enter__(self):
                return self

            def __exit__(self, *exc):
                return False

            def create_dataset(self, key, data=None):
                class DS:
                    attrs = seen.setdefault(key, {})
                return DS

    root = str(tmp_path)
    mixture_directory(root)
    table = str(tmp_path / "chem.txt")
    chem = small_table()
    with open(table, "w") as fh:
        fh.write("T(K) P(bar) H2O CH4 CO\n")
        for i in range(6):
            fh.write(" ".join(repr(float(v)) for v in (chem["temperature"][i], np.log10(chem["pressure"][i]), chem["H2O"][i],
                                                       chem["CH4"][i], chem["CO"][i])) + "\n")
    calls = []
    monkeypatch.setattr(of, "compute_ck_of_sums", fake_device(calls))
    monkeypatch.setattr(optics, "_h5py", lambda: Recorder)
    of.compute_ck_premixed(GASES, root, table, new_wno=[105.0], new_dwno=[4.0], climate_filename="x.hdf5", verbose=False)
    # the file goes through the reader, row file_number - 1 (pandas' fast float parser keeps about 16 digits)
    assert np.allclose(calls[0]["weights"][0], [chem[g][2] for g in GASES], rtol=1e-9, atol=0.0)
    assert seen["file"] == {"chemistry_file": table}
    assert seen["pressures"]["description"] == "bars" and seen["kcoeffs"]["description"].startswith("k coefficients")
    assert seen["abunds"]["description"].startswith("matrix of abundances in v/v units")
    assert seen["abunds_map"]["description"] == "array of strings that defines the order of abunds key"
    assert seen["ck_molecules"]["description"] == "molecules included in the ck weighted table"
    assert len(seen) == 12


def test_compute_sum_molecular_writes_the_header_then_one_sum_per_point(tmp_path, monkeypatch, h5py, capsys):
    root = str(tmp_path / "xsec")
    pres, temp, file_numbers, numw, delwn, start = mixture_directory(root)
    chem = small_table()
    calls = []

    def fake_sum(rows, weights, grids=None, out_grid=None, out="host"):
        calls.append((len(rows), np.array(weights), grids, np.array(out_grid), out))
        return sum(w * np.asarray(rows[m]) for m, w in enumerate(weights))

    monkeypatch.setattr(of, "weighted_sum", fake_sum)
    of.compute_sum_molecular(GASES, root, chem, str(tmp_path), "sums.hdf5", new_wno=[1.0], new_dwno=[1.0])
    with h5py.File(str(tmp_path / "sums.hdf5"), "r") as f:
        keys = list(f.keys())
        assert keys[:6] == ["ck_molecules", "pressure_bar", "temperature_K", "file_number", "abunds", "abunds_map"]
        assert keys[6:] == ["sum_%d" % i for i in file_numbers]
        assert [x.decode("utf-8") for x in f["ck_molecules"][:]] == GASES
        assert [x.decode("utf-8") for x in f["abunds_map"][:]] == list(chem)
        assert np.array_equal(f["pressure_bar"][:], pres) and np.array_equal(f["temperature_K"][:], temp)
        assert np.array_equal(f["file_number"][:], file_numbers) and f["abunds"][:].shape == (6, 5)
        for i in file_numbers:
            want = sum(chem[g][i - 1] * (100.0 * m + i) for m, g in enumerate(GASES))
            assert f["sum_%d" % i][:].shape == (numw[i - 1],) and np.all(f["sum_%d" % i][:] == want)
    assert all(c[0] == 3 and c[2] is None and c[4] == "host" for c in calls)
    assert np.array_equal(calls[0][3], np.arange(numw[2]) * delwn[2] + start[2])
    printed = [p for p in capsys.readouterr().out.split("\n") if p]
    assert printed[0].split() == ["completed", "3", "0.001", "500.0"] and len(printed) == 6


def test_refusals_and_re_exports(tmp_path, monkeypatch):
    root = str(tmp_path)
    mixture_directory(root)
    chem = small_table()
    calls = []
    monkeypatch.setattr(of, "compute_ck_of_sums", fake_device(calls))
    monkeypatch.setattr(of, "weighted_sum", lambda *a, **k: calls.append(a))
    grid = dict(new_wno=[1.0], new_dwno=[1.0], verbose=False)
    assert jdi.compute_ck_premixed is of.compute_ck_premixed and jdi.weighted_sum is not None
    assert jdi.compute_sum_molecular is of.compute_sum_molecular
    with pytest.raises(Exception, match="compute_ck_premixed: .*grid1460.csv does not exist"):
        of.compute_ck_premixed(GASES, str(tmp_path / "nowhere"), chem, **grid)
    with pytest.raises(NotImplementedError, match="compute_ck_premixed: the alkali"):
        of.compute_ck_premixed(["H2O", "Na"], root, chem, **grid)
    with pytest.raises(NotImplementedError, match="HDF5"):
        of.compute_ck_premixed(["H2O", "feh_000.hdf5"], root, chem, **grid)
    with pytest.raises(Exception, match="holds neither 3.npy .* nor p_3"):
        os.makedirs(os.path.join(root, "NH3"))
        of.compute_ck_premixed(["H2O", "NH3"], root, chem, **grid)
    with pytest.raises(Exception, match="no column for TiO"):
        write_directory(root, "TiO", [np.ones(40)] * 6, [1.0] * 6, [1.0] * 6, range(1, 7), [40] * 6, [1.0] * 6, [0.0] * 6)
        mixture_directory(root)
        of.compute_ck_premixed(["H2O", "TiO"], root, chem, **grid)
    with pytest.raises(Exception, match="wv_file_name, or new_wno and new_dwno, or min_max_wavelength and R"):
        of.compute_ck_premixed(GASES, root, chem, verbose=False)
    with pytest.raises(Exception, match="names no gas"):
        of.compute_ck_premixed([], root, chem, **grid)
    open(os.path.join(root, "CH4", "readomni.fits"), "w").close()
    with pytest.raises(NotImplementedError, match="astropy"):
        of.compute_ck_premixed(GASES, root, chem, **grid)
    os.remove(os.path.join(root, "CH4", "readomni.fits"))
    open(os.path.join(root, "CO", "wavelengths.txt"), "w").close()
    with pytest.raises(NotImplementedError, match="compute_sum_molecular: the Lupu"):
        monkeypatch.setattr(optics, "_h5py", lambda: None)
        of.compute_sum_molecular(GASES, root, chem, root, "s.hdf5")
    os.remove(os.path.join(root, "CO", "wavelengths.txt"))
    monkeypatch.undo()
    monkeypatch.setattr(of, "compute_ck_of_sums", fake_device(calls))
    monkeypatch.setattr(of, "weighted_sum", lambda *a, **k: calls.append(a))
    monkeypatch.setitem(sys.modules, "h5py", None)                  # said before the work, not after it
    with pytest.raises(Exception, match="needs the h5py package"):
        of.compute_sum_molecular(GASES, root, chem, root, "s.hdf5", verbose=False)
    with pytest.raises(Exception, match="needs the h5py package"):
        of.compute_ck_premixed(GASES, root, chem, climate_filename=os.path.join(root, "t.hdf5"), **grid)
    assert not calls and not os.path.exists(os.path.join(root, "s.hdf5"))
    # weighted_sum's own arguments, before the device is touched
    monkeypatch.undo()
    rows = [np.ones(4), np.ones(4)]
    for kwargs, msg in ((dict(weights=[1.0]), "2 rows need 2 weights"), (dict(weights=[1.0, np.nan]), "finite"),
                        (dict(weights=[1.0, np.inf]), "finite"), (dict(weights=[1.0, 2.0], out="disk"), "'host' or 'device'"),
                        (dict(weights=[1.0, 2.0], grids=[np.arange(4.0)] * 2), "need out_grid"),
                        (dict(weights=[1.0, 2.0], grids=[np.arange(4.0)], out_grid=np.arange(4.0)), "1 grids for 2 rows")):
        with pytest.raises(Exception, match=msg):
            of.weighted_sum(rows, **kwargs)
    with pytest.raises(Exception, match="non-empty sequence"):
        of.weighted_sum([], [])
    assert of.are_arrays_different(np.arange(3.0), np.arange(4.0)) and not of.are_arrays_different(np.arange(3.0), np.arange(3.0))
    assert of.are_arrays_different(np.arange(3.0), np.arange(3.0) + 1e-12)
