"""Generate tests/golden/continuum_factory.npz by running the REFERENCE's own opacity factory (build container only):

    python tests/golden/make_continuum_factory.py

The reference's ``opacity_factory`` module does not import here (astropy, h5py), so its functions are taken from its file
with ``ast`` and compiled at generation time next to numpy, scipy and pandas; none of their text is stored.  Taken:
``get_original_data``, ``restructure_opacity``, ``insert``, ``h2h2_overtone``, ``fit_linsky``, ``get_h2minus``,
``get_hminusbf``, ``get_hminusff``, ``find_nearest``, ``find_nearest_1d``, ``adapt_array``, ``convert_array``, ``open_local``,
``build_skeleton``, ``create_grid`` and ``insert_molecular_1460``.

The file holds inputs and outputs only:
  meta/numpy, meta/scipy, meta/pandas   the versions that wrote it
  overtone/wno, temps, values           the numbers of $picaso_refdata/opacities/H2H2_ov2_eq.tbl as pandas reads them
  h2minus/theta, lam, values            the numbers of $picaso_refdata/opacities/h2minus.csv likewise
  temperatures                          the nine temperatures of the synthetic CIA tables
  cia/<table>/old_wno, log1e4           two tables: the grid, and round(1e4 log10 opacity) as int32, (ntemp, 2, nold), pairs
                                        H2H2 and H2He; the CIA file prints log1e4 / 1e4 with four decimals.  "gaps": the
                                        issue's table (0 .. 9980 in steps of 20; -33 below 100, in 4000 .. 4200 and above
                                        9000 in H2H2); "full": 0 .. 12980 without a placeholder from 100 up
  grid/<a..f>                           the new grids
  rows/<grid>                           what restructure_opacity inserted, (ntemp, nspecies, nwno), species H2H2, H2He, H2-,
                                        H-bf, H-ff; for the fine grid c and for d (the "full" table on grid b) H2H2 alone
  src/<name>/<T>                        the five source functions on grid a at 300, 800 and 2500 K
  mol/...                               the molecular part: grid1460.csv's columns, three rows of 5 001 points, and what the
                                        reference's insert_molecular_1460 inserted for new_R, new_dwno and insert_direct
                                        (its file-type test wants more than 1 000 files: it is shown a glob that repeats
                                        the three)
"""
import ast
import glob as real_glob
import io
import math
import os
import sqlite3
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

TEMPERATURES = np.array([75., 300., 400., 599., 600., 799., 800., 1000., 2500.])
COLNAMES = ["wno", "H2H2", "H2He"]
NAMES = ["get_original_data", "restructure_opacity", "insert", "h2h2_overtone", "fit_linsky", "get_h2minus", "get_hminusbf",
         "get_hminusff", "find_nearest", "find_nearest_1d", "adapt_array", "convert_array", "open_local", "build_skeleton",
         "create_grid", "insert_molecular_1460"]


def new_grids():
    return {"a": np.geomspace(300, 60000, 900), "b": np.arange(400, 13000, 14.0), "c": np.arange(9000, 12500, 0.9),
            "e": np.arange(500, 9900, 47.0), "f": np.array([5000.0, 10500.0])}


def cia_tables():
    """``{name: (old_wno, log1e4 int32 (ntemp, 2, nold))}``."""
    out = {}
    for name, top in (("gaps", 9980), ("full", 12980)):
        w = np.arange(0.0, top + 1, 20.0)
        tab = np.empty((TEMPERATURES.size, 2, w.size), dtype=np.int32)
        for i, t in enumerate(TEMPERATURES):
            h2h2 = -6.0 - 1.5e-4 * w + 0.8 * np.sin(w / 700.0 + i) - 30.0 / np.sqrt(t)
            h2he = -6.5 - 1.2e-4 * w + 0.6 * np.cos(w / 900.0 - i) - 25.0 / np.sqrt(t)
            h2h2[w < 100] = -33.0
            h2he[w == 0] = -33.0
            if name == "gaps":
                h2h2[(w >= 4000) & (w <= 4200)] = -33.0
                h2h2[w > 9000] = -33.0
            tab[i, 0], tab[i, 1] = np.round(h2h2 * 1e4), np.round(h2he * 1e4)
        out[name] = (w, tab)
    return out


def write_cia_file(path, old_wno, log1e4):
    """The CIA file of the reference's get_original_data: ``nwno ntemp``, then per temperature its line and the rows."""
    with open(path, "w") as fh:
        fh.write("%d %d\n" % (old_wno.size, TEMPERATURES.size))
        for i, t in enumerate(TEMPERATURES):
            fh.write("%.0f.\n" % t)
            for j, w in enumerate(old_wno):
                fh.write("%.1f  %.4f  %.4f\n" % (w, log1e4[i, 0, j] / 1e4, log1e4[i, 1, j] / 1e4))


def molecular_inputs():
    """grid1460.csv's columns and three rows of 5 001 points: a few distinct values, zeros and values below the floor."""
    csv = dict(pressure_bar=np.array([1e-3, 1.0, 1.0]), temperature_K=np.array([300.0, 300.0, 900.0]),
               file_number=np.array([1, 2, 3]), number_wave_pts=np.array([5001, 5001, 5001]),
               delta_wavenumber=np.array([0.5, 0.5, 0.4]), start_wavenumber=np.array([2000.0, 2000.0, 2100.0]))
    j = np.arange(5001)
    rows = np.stack([(((j * 7919 + r * 104729) % 1009) + 1) * 1e-24 for r in range(3)])
    rows[:, j % 97 == 0] = 0.0
    rows[:, j % 89 == 0] = 1e-120
    rows[:, 1000:1040:2], rows[:, 1001:1040:2] = 0.0, 1e-120         # a run below the floor: new points fall inside it
    return csv, rows


def write_directory(root, form, csv, rows, molecule="H2O"):
    os.makedirs(os.path.join(root, molecule))
    keys = list(csv)
    with open(os.path.join(root, "grid1460.csv"), "w") as fh:
        fh.write(",".join(keys) + "\n")
        for k in range(len(csv["file_number"])):
            fh.write(",".join(repr(csv[c][k].item()) for c in keys) + "\n")
    for k, i in enumerate(csv["file_number"]):
        if form == "npy":
            np.save(os.path.join(root, molecule, "%d.npy" % i), rows[k])
        else:
            rows[k].tofile(os.path.join(root, molecule, "p_%d" % i))


MOL_MODES = {"new_R": dict(new_R=1000.0, old_R=20000.0), "new_dwno": dict(new_dwno=1.0, old_dwno=0.05),
             "insert_direct": dict(insert_direct=True)}
MOL_RANGE = (2.3, 4.9)                  # micron: beyond both ends of the third row


def _reference():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pandas as pd
    import ref_shim
    import scipy.signal as sig
    refdata = os.path.join(ref_shim.REF_ROOT, "reference")
    os.environ["picaso_refdata"] = refdata
    fake_glob = types.SimpleNamespace(glob=lambda pattern: real_glob.glob(pattern) * 1001)
    ns = {"np": np, "pd": pd, "os": os, "sig": sig, "sqlite3": sqlite3, "io": io, "glob": fake_glob, "math": math,
          "__refdata__": refdata}
    path = os.path.join(ref_shim.REF_ROOT, "picaso", "opacity_factory.py")
    with open(path) as fh:
        body = ast.parse(fh.read(), path).body
    nodes = [n for n in body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert sorted(set(n.name for n in nodes)) == sorted(NAMES)
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
    return ns, pd, refdata


def main():
    import scipy
    ns, pd, refdata = _reference()
    sys.path.insert(0, ROOT)
    from picaso_amd import opacity_factory as opf
    store = {"meta/numpy": np.array(np.__version__), "meta/scipy": np.array(scipy.__version__),
             "meta/pandas": np.array(pd.__version__), "temperatures": TEMPERATURES}

    # ---- the two data tables, as the reference's functions read them with pandas; the package's readers agree
    df = pd.read_csv(os.path.join(refdata, "opacities", "H2H2_ov2_eq.tbl"), sep=r"\s+").set_index("wavenumber")
    ov = (np.array(df.index, dtype=float), np.array([float(c) for c in df.keys()]), df.values.astype(float))
    df = pd.read_csv(os.path.join(refdata, "opacities", "h2minus.csv"), skiprows=5, header=0).set_index("theta")
    bell = (df.index.values.astype(float), df.columns.astype(float).values, df.values.astype(float))
    for mine, theirs in ((opf.read_overtone_table(), ov), (opf.read_h2minus_table(), bell)):
        assert all(np.array_equal(x, y) for x, y in zip(mine, theirs))
    store["overtone/wno"], store["overtone/temps"], store["overtone/values"] = ov
    store["h2minus/theta"], store["h2minus/lam"], store["h2minus/values"] = bell
    assert 10 ** np.array([-33.0])[0] == 1e-33

    # ---- the continuum rows
    grids = new_grids()
    tables = cia_tables()
    for g, w in grids.items():
        store["grid/" + g] = w
    work = tempfile.mkdtemp()
    runs = [(g, "gaps", g not in ("c",)) for g in grids] + [("d", "full", False)]
    grids["d"] = grids["b"]
    for name, (old_wno, log1e4) in tables.items():
        store["cia/%s/old_wno" % name], store["cia/%s/log1e4" % name] = old_wno, log1e4
        write_cia_file(os.path.join(work, name + ".txt"), old_wno, log1e4)
    smoothed = {}
    for g, table, all_species in runs:
        db = os.path.join(work, "ref_%s.db" % g)
        ns["build_skeleton"](db)
        og, temps, old_wno, molecules = ns["get_original_data"](os.path.join(work, table + ".txt"), COLNAMES, db)
        assert np.array_equal(temps, TEMPERATURES) and np.array_equal(old_wno, tables[table][0]) and molecules == COLNAMES[1:]
        for k, m in enumerate(molecules):      # the file's four decimals parse to the quotient
            assert np.array_equal(og[m].values.reshape(TEMPERATURES.size, -1), tables[table][1][:, k] / 1e4)
        ns["restructure_opacity"](db, len(temps), temps, molecules, og, old_wno, grids[g].copy())
        cur, conn = ns["open_local"](db)
        cur.execute("SELECT molecule, temperature, opacity FROM continuum ORDER BY id")
        got = cur.fetchall()
        conn.close()
        species = molecules + ["H2-", "H-bf", "H-ff"]
        assert [r[0] for r in got] == species * TEMPERATURES.size
        assert [r[1] for r in got] == [float(t) for t in np.repeat(TEMPERATURES, 5)]
        block = np.stack([r[2] for r in got]).reshape(TEMPERATURES.size, 5, -1)
        store["rows/" + g] = block if all_species else block[:, :1]
        # which rows the reference smoothed: the package's host rows without the filter differ there
        plain = opf.continuum_rows_numpy(tables[table][1] / 1e4, TEMPERATURES, old_wno, molecules, grids[g], ov, bell,
                                         smooth=False)
        mine = opf.continuum_rows_numpy(tables[table][1] / 1e4, TEMPERATURES, old_wno, molecules, grids[g], ov, bell)
        assert np.array_equal(mine, block, equal_nan=True), g
        smoothed[g] = [bool(np.any(plain[i, 0] != block[i, 0])) for i in range(TEMPERATURES.size)]
    # every branch the issue names is hit
    w = grids["a"]
    assert smoothed["a"] == [True] * 9 and np.sum((w > 9950) & (w < 11200)) == 20 and opf.smoothing_window(w) == 51
    assert np.all(store["rows/a"][:, 0, (w > 9950) & (w < 11200)] == 0.0)
    assert opf.smoothing_window(grids["b"]) == 7 and np.sum((grids["b"] > 9950) & (grids["b"] < 11200)) == 89
    assert opf.smoothing_window(grids["c"]) == 101 and np.sum((grids["c"] > 9950) & (grids["c"] < 11200)) == 1389
    assert all(smoothed["b"]) and all(smoothed["c"]) and not any(smoothed["d"]) and not any(smoothed["e"])
    wave = 1e4 / w
    assert np.any(wave > 20) and np.any(wave < 0.1823) and np.any((wave > 0.1823) & (wave <= 0.3645)) and np.any(wave > 0.3645)
    assert np.any(w > 1e4 / 1.6419) and np.any(w < 1e4 / 1.6419)
    for T in (300.0, 800.0, 2500.0):
        t = np.float64(T)
        h, loc, add = ns["h2h2_overtone"](t, w.copy())
        assert add == (T <= 350)
        if add:
            store["src/overtone/%d" % T], store["src/overtone_loc/%d" % T] = h, loc[0]
        store["src/linsky/%d" % T] = ns["fit_linsky"](t, w.copy())
        store["src/h2minus/%d" % T] = ns["get_h2minus"](t, w.copy())
        store["src/hminusff/%d" % T] = ns["get_hminusff"](t, w.copy())
    store["src/hminusbf/0"] = ns["get_hminusbf"](w.copy())

    # ---- the molecular part
    csv, rows = molecular_inputs()
    for c, v in csv.items():
        store["mol/csv/" + c] = v
    store["mol/rows"] = rows
    for form in ("npy", "p_"):
        root = os.path.join(work, "xsec_" + form.strip("_"))
        write_directory(root, form, csv, rows)
        for mode, kw in MOL_MODES.items():
            db = os.path.join(work, "mol_%s_%s.db" % (form.strip("_"), mode))
            ns["build_skeleton"](db)
            grid = ns["insert_molecular_1460"]("H2O", MOL_RANGE[0], MOL_RANGE[1], root, db, **kw)
            cur, conn = ns["open_local"](db)
            cur.execute("SELECT ptid, molecule, temperature, pressure, opacity FROM molecular ORDER BY id")
            got = cur.fetchall()
            cur.execute("SELECT wavenumber_grid FROM header")
            header = cur.fetchone()[0]
            conn.close()
            assert [r[0] for r in got] == [1, 2, 3] and np.array_equal(header, grid)
            if form == "npy":
                store["mol/%s/grid" % mode] = grid
                for r in got:
                    store["mol/%s/row%d" % (mode, r[0])] = r[4]
                assert all(np.any(r[4] == 1e-100) for r in got)
            else:
                assert all(np.array_equal(r[4], store["mol/%s/row%d" % (mode, r[0])]) for r in got)

    path = os.path.join(HERE, "continuum_factory.npz")
    np.savez_compressed(path, **store)
    size = os.path.getsize(path)
    print("wrote", path, "%.1f KB" % (size / 1024), {g: sum(s) for g, s in smoothed.items()})
    assert size <= 1000 * 1000, "the fixture stays under 1 MB"


if __name__ == "__main__":
    main()
