"""Generate tests/golden/chemistry.npz (parts 1, 2 and 4 below) and tests/golden/chemistry/ (the cut-down files, and part 3
as ``expected.npz``: one file would pass the repository's limit of 1 MiB per file) by running the REFERENCE's own source
(build container only):

    python tests/golden/make_chemistry.py

Everything written is data: arrays, names and cut-down copies of the reference's plain-text chemistry tables.

1. Full tables as arrays: ``sonora_2121grid_feh0.0_co0.55.txt`` (``t2121/<column>``) and ``2015_06_1060grid_feh_00_co_10.txt``
   (``t1060/<column>``) and ``visscher_abunds_m+0.0_co1.0`` (``tlow/<column>``), read as the reference reads them (pandas),
   with the column order in ``t2121/columns``, ``t1060/columns``, ``tlow/columns``.

2. Cut-down copies for the readers, under tests/golden/chemistry/: the header and the rows of the first two temperatures
   of seven 2121 files (``visscher_grid_2121/``, names that span feh and co), of one 1060 file (``visscher_grid_1060/``) and
   of ``visscher_abunds_m+0.0_co1.0``; the columns the reference reads from the cut-down 2121, 1060 and low-grid files are
   stored as ``cut2121/...``, ``cut1060/...``, ``cutlow/...``.

3. Expected values from the reference's own ``inputs.chem_interp`` behind ``chemeq_visscher_2121(0.55, 0.0)``,
   ``chemeq_visscher_1060(1.0, 0.0)`` and ``channon_grid_low()`` with ``__refdata__`` on the reference's data:
   * ``hj``: 61 levels of ``base_cases/HJ.pt`` (the file holds 90; 61 of them, evenly spread from the top to the bottom);
   * ``scatter``: 500 points run as one profile -- exact grid nodes, points below and above the 2121 table in T and in P,
     points in the first and last cell of each axis, the rest random;
   * ``facets``: 12 levels x 3 x 2 facets, computed column by column (what ``chemeq_3d`` must reproduce; the reference's own
     ``chemeq_3d`` needs xarray).
   Keys: ``<case>/temperature``, ``<case>/pressure``, ``<case>/<grid>/<species>`` with grid in ``2121``, ``1060``, ``low``.

4. The file the reference selects: for 2121 in the cut-down directory, targets ``sel2121/targets`` (cto_absolute, log_mh) ->
   ``sel2121/chosen``; the last target is a tie between two files (same distance, same |dfeh|, same |dco|), which the
   reference leaves to ``os.listdir`` order: asserted here that it returns one of the two, stored is the first in sorted
   order.  For 1060 in the reference's directory, ``sel1060/targets`` (c_o, log_mh) -> ``sel1060/chosen``, an exception's
   message where the reference raises.
"""
import contextlib
import io
import os
import shutil
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_shim  # noqa: E402
from make_diseq import import_justdoit  # noqa: E402

OUT_DIR = os.path.join(HERE, "chemistry")
FILE_2121 = "sonora_2121grid_feh0.0_co0.55.txt"
FILE_1060 = "2015_06_1060grid_feh_00_co_10.txt"
FILE_LOW = "visscher_abunds_m+0.0_co1.0"
CUT_2121 = [FILE_2121, "sonora_2121grid_feh0.5_co0.55.txt", "sonora_2121grid_feh-0.5_co0.55.txt",
            "sonora_2121grid_feh0.0_co0.27.txt", "sonora_2121grid_feh0.0_co1.10.txt", "sonora_2121grid_feh1.0_co0.82.txt",
            "sonora_2121grid_feh2.0_co0.14.txt"]
# (cto_absolute, log_mh): an exact hit, an off-grid target, targets beyond the grid, and the tie (feh 0.25 between 0.0 and 0.5)
TARGETS_2121 = [(0.55, 0.0), (0.6, 0.1), (0.3, -0.1), (0.9, 0.8), (3.0, 5.0), (0.1, -3.0), (0.55, 0.25)]
TIE_2121 = ["sonora_2121grid_feh0.0_co0.55.txt", "sonora_2121grid_feh0.5_co0.55.txt"]
# (c_o, log_mh): an exact hit, off-grid targets, targets below the lists, and the two exceptions
TARGETS_1060 = [(1.0, 0.0), (1.2, 0.4), (0.1, -1.0), (2.3, 1.6), (1.0, 2.5), (3.0, 0.0)]


def cut_down(src, dst, header_lines=1, sep=None):
    """The header and the rows of the first two temperatures."""
    with open(src) as fh:
        lines = fh.readlines()
    head, rows = lines[:header_lines], lines[header_lines:]
    if sep is None:
        temp = lambda ln: ln.split()[0]                                # noqa: E731
    else:
        col = head[0].rstrip("\r\n").split(sep).index("temperature")
        temp = lambda ln: ln.rstrip("\r\n").split(sep)[col]            # noqa: E731
    seen, keep = [], []
    for ln in rows:
        t = temp(ln)
        if t not in seen:
            if len(seen) == 2:
                break
            seen.append(t)
        keep.append(ln)
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w") as fh:
        fh.writelines(head + keep)


def bundle(jdi, t, p):
    b = object.__new__(jdi.inputs)
    b.inputs = {"atmosphere": {"profile": pd.DataFrame({"temperature": np.array(t, dtype=float),
                                                        "pressure": np.array(p, dtype=float)})}}
    return b


def run(jdi, grid, t, p):
    """The reference's abundances of one profile, rows in the order given (chem_interp does not sort)."""
    b = bundle(jdi, t, p)
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        if grid == "2121":
            b.chemeq_visscher_2121(0.55, log_mh=0.0)
        elif grid == "1060":
            b.chemeq_visscher_1060(1.0, 0.0)
        else:
            b.channon_grid_low()
    prof = b.inputs["atmosphere"]["profile"]
    assert np.array_equal(prof["temperature"].values, t) and np.array_equal(prof["pressure"].values, p)
    return {k: np.array(prof[k].values, dtype=float) for k in prof.keys() if k not in ("temperature", "pressure")}


def scatter_points(tab):
    """500 points against the 2121 table: nodes, off-table points, first and last cells, then random ones."""
    temps, press = np.unique(tab["temperature"]), np.unique(tab["pressure"])
    rng = np.random.default_rng(20261020)
    t, p = [], []
    for it in (0, 1, 50, len(temps) - 2, len(temps) - 1):              # exact nodes
        for ip in (0, 1, 10, len(press) - 2, len(press) - 1):
            t.append(temps[it])
            p.append(press[ip])
    for tv in (0.3 * temps[0], 0.9 * temps[0], 1.1 * temps[-1], 3.0 * temps[-1]):      # off the table in T
        for pv in (press[0] * 1e-3, press[3] * 1.7, press[-1] * 50.0):                  # and in P
            t.append(tv)
            p.append(pv)
    for pv in (press[0] * 1e-2, press[0] * 0.5, press[-1] * 2.0, press[-1] * 1e3):
        t.append(rng.uniform(temps[0], temps[-1]))
        p.append(pv)
    for _ in range(20):                                                # first and last cell of each axis
        t.append(rng.uniform(temps[0], temps[1]))
        p.append(10 ** rng.uniform(np.log10(press[0]), np.log10(press[-1])))
        t.append(rng.uniform(temps[-2], temps[-1]))
        p.append(10 ** rng.uniform(np.log10(press[0]), np.log10(press[-1])))
        t.append(rng.uniform(temps[0], temps[-1]))
        p.append(10 ** rng.uniform(np.log10(press[0]), np.log10(press[1])))
        t.append(rng.uniform(temps[0], temps[-1]))
        p.append(10 ** rng.uniform(np.log10(press[-2]), np.log10(press[-1])))
    n = 500 - len(t)
    t += list(rng.uniform(0.8 * temps[0], 1.1 * temps[-1], n))
    p += list(10 ** rng.uniform(np.log10(press[0]) - 1, np.log10(press[-1]) + 1, n))
    return np.array(t), np.array(p)


class ReadSpy:
    """Records the paths handed to pandas.read_csv."""

    def __init__(self):
        self.paths, self.real = [], pd.read_csv

    def __enter__(self):
        def spy(path, *a, **k):
            self.paths.append(path)
            return self.real(path, *a, **k)
        pd.read_csv = spy
        return self

    def __exit__(self, *exc):
        pd.read_csv = self.real


def main():
    jdi = import_justdoit()
    ref = os.path.join(ref_shim.REF_ROOT, "reference")
    chem = os.path.join(ref, "chemistry")
    assert jdi.__refdata__ == ref, jdi.__refdata__
    store = {}

    # 1. full tables
    full = {}
    for tag, path, names in (("t2121", os.path.join(chem, "visscher_grid_2121", FILE_2121), ("T(K)", "P(bar)")),
                             ("t1060", os.path.join(chem, "visscher_grid_1060", FILE_1060), ("T (K)", "P (bar)"))):
        header = pd.read_csv(path).keys()[0]
        cols = header.replace(names[0], "temperature").replace(names[1], "pressure").split()
        a = pd.read_csv(path, sep=r"\s+", skiprows=1, header=None, names=cols)
        a["pressure"] = 10 ** a["pressure"]
        full[tag] = a
        store[tag + "/columns"] = np.array(cols, dtype="U16")
        for k in cols:
            store["%s/%s" % (tag, k)] = np.array(a[k].values, dtype=float)
    a = pd.read_csv(os.path.join(chem, FILE_LOW)).iloc[:, 1:]
    store["tlow/columns"] = np.array(list(a.keys()), dtype="U16")
    for k in a.keys():
        store["tlow/" + k] = np.array(a[k].values, dtype=float)
    io_utils = __import__("picaso.io_utils", fromlist=["read_visscher_2121"])
    same = io_utils.read_visscher_2121(os.path.join(chem, "visscher_grid_2121", FILE_2121))
    assert all(np.array_equal(same[k].values, full["t2121"][k].values) for k in same.keys())

    # 2. cut-down copies
    if os.path.isdir(OUT_DIR):
        shutil.rmtree(OUT_DIR)
    for name in CUT_2121:
        cut_down(os.path.join(chem, "visscher_grid_2121", name), os.path.join(OUT_DIR, "visscher_grid_2121", name))
    cut_down(os.path.join(chem, "visscher_grid_1060", FILE_1060), os.path.join(OUT_DIR, "visscher_grid_1060", FILE_1060))
    cut_down(os.path.join(chem, FILE_LOW), os.path.join(OUT_DIR, FILE_LOW), sep=",")
    cut = io_utils.read_visscher_2121(os.path.join(OUT_DIR, "visscher_grid_2121", FILE_2121))
    store["cut2121/columns"] = np.array(list(cut.keys()), dtype="U16")
    for k in cut.keys():
        store["cut2121/" + k] = np.array(cut[k].values, dtype=float)
    path = os.path.join(OUT_DIR, "visscher_grid_1060", FILE_1060)
    header = pd.read_csv(path).keys()[0]
    cols = header.replace("T (K)", "temperature").replace("P (bar)", "pressure").split()
    a = pd.read_csv(path, sep=r"\s+", skiprows=1, header=None, names=cols)
    a["pressure"] = 10 ** a["pressure"]
    store["cut1060/columns"] = np.array(cols, dtype="U16")
    for k in cols:
        store["cut1060/" + k] = np.array(a[k].values, dtype=float)
    a = pd.read_csv(os.path.join(OUT_DIR, FILE_LOW)).iloc[:, 1:]
    store["cutlow/columns"] = np.array(list(a.keys()), dtype="U16")
    for k in a.keys():
        store["cutlow/" + k] = np.array(a[k].values, dtype=float)

    # 3. expected values
    hj = pd.read_csv(os.path.join(ref, "base_cases", "HJ.pt"), sep=r"\s+")
    rows = np.round(np.linspace(0, len(hj) - 1, 61)).astype(int)
    assert len(np.unique(rows)) == 61
    cases = {"hj": (hj["temperature"].values[rows].astype(float), hj["pressure"].values[rows].astype(float)),
             "scatter": scatter_points(full["t2121"])}
    for name, (t, p) in cases.items():
        store[name + "/temperature"], store[name + "/pressure"] = t, p
        for grid in ("2121", "1060", "low"):
            for k, v in run(jdi, grid, t, p).items():
                store["%s/%s/%s" % (name, grid, k)] = v
        print("%-8s %d points" % (name, len(t)))
    rng = np.random.default_rng(7)
    p12 = np.logspace(-5, 2, 12)
    t12 = 700.0 + 900.0 * (np.log10(p12) + 5) / 7
    t3d = t12[:, None, None] * (1.0 + 0.15 * rng.uniform(-1, 1, (1, 3, 2))) + rng.uniform(-30, 30, (12, 3, 2))
    store["facets/temperature"], store["facets/pressure"] = t3d, p12
    out = {}
    for ig in range(3):
        for it in range(2):
            for k, v in run(jdi, "2121", t3d[:, ig, it].copy(), p12).items():
                out.setdefault(k, np.zeros((12, 3, 2)))[:, ig, it] = v
    for k, v in out.items():
        store["facets/2121/" + k] = v

    # 4. file selection
    chosen = []
    jdi.__refdata__ = os.path.dirname(OUT_DIR)                         # tests/golden: chemistry/visscher_grid_2121 below it
    try:
        for i, (co, mh) in enumerate(TARGETS_2121):
            with ReadSpy() as spy, contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
                bundle(jdi, [1000.0, 1100.0], [0.1, 1.0]).chemeq_visscher_2121(co, log_mh=mh)
            name = os.path.basename(spy.paths[0])
            if i == len(TARGETS_2121) - 1:
                assert name in TIE_2121, name
                print("tie: the reference took %s (os.listdir order); stored: %s" % (name, sorted(TIE_2121)[0]))
                name = sorted(TIE_2121)[0]
            chosen.append(name)
            print("2121 target co %-5s feh %-5s -> %s" % (co, mh, name))
    finally:
        jdi.__refdata__ = ref
    store["sel2121/targets"] = np.array(TARGETS_2121)
    store["sel2121/chosen"] = np.array(chosen, dtype="U64")
    chosen = []
    for co, mh in TARGETS_1060:
        try:
            with ReadSpy() as spy, contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
                bundle(jdi, [1000.0, 1100.0], [0.1, 1.0]).chemeq_visscher_1060(co, mh)
            chosen.append(os.path.basename(spy.paths[0]))
        except Exception as e:
            chosen.append("raises: " + str(e))
        print("1060 target co %-5s feh %-5s -> %s" % (co, mh, chosen[-1]))
    store["sel1060/targets"] = np.array(TARGETS_1060)
    store["sel1060/chosen"] = np.array(chosen, dtype="U64")
    assert sum(c.startswith("raises") for c in chosen) == 2

    # two files, each below the repository's limit of 1 MiB per file: the tables, and what the reference makes of them
    expected = {k: store.pop(k) for k in list(store) if k.split("/")[0] in ("hj", "scatter", "facets")}
    for path, part in ((os.path.join(HERE, "chemistry.npz"), store), (os.path.join(OUT_DIR, "expected.npz"), expected)):
        np.savez_compressed(path, **part)
        print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))
        assert os.path.getsize(path) < 2 ** 20
    for d, _, files in os.walk(OUT_DIR):
        for f in files:
            print("  %s %.1f KB" % (os.path.relpath(os.path.join(d, f), HERE), os.path.getsize(os.path.join(d, f)) / 1024))


if __name__ == "__main__":
    main()
