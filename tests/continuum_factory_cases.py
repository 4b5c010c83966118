"""What the host and the GPU tests of the opacity-database factory share: tests/golden/continuum_factory.npz (written by
tests/golden/make_continuum_factory.py from the reference's own functions), the synthetic CIA files and cross-section
directories the fixture's arrays describe, and the tolerances of DESIGN section 5q."""
import functools
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_continuum_factory", os.path.join(HERE, "golden", "make_continuum_factory.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

COLNAMES, MOLECULES, SPECIES = gen.COLNAMES, gen.COLNAMES[1:], gen.COLNAMES[1:] + ["H2-", "H-bf", "H-ff"]
# grid -> (CIA table, species stored)
RUNS = {"a": ("gaps", 5), "b": ("gaps", 5), "c": ("gaps", 1), "d": ("full", 1), "e": ("gaps", 5), "f": ("gaps", 5)}
U = 2.0 ** -53
# DESIGN section 5q, in ulp of the reference value (np.spacing): 10**x as cheminterp.hip documents; the Linsky exp branch
# and H-bf derived there; everything else bit for bit
ULP_EXP10, ULP_LINSKY, ULP_HBF = 4, 8, 8


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(os.path.join(HERE, "golden", "continuum_factory.npz")) as z:
        return {k: z[k] for k in z.files}


def tables():
    f = fixture()
    return ((f["overtone/wno"], f["overtone/temps"], f["overtone/values"]),
            (f["h2minus/theta"], f["h2minus/lam"], f["h2minus/values"]))


def grid(g):
    return fixture()["grid/" + ("b" if g == "d" else g)]


def cia(table):
    """``(old_wno, log10 opacity (ntemp, 2, nold))``: the quotients the CIA file's four decimals parse to."""
    f = fixture()
    return f["cia/%s/old_wno" % table], f["cia/%s/log1e4" % table] / 1e4


def write_cia(path, table):
    f = fixture()
    gen.write_cia_file(str(path), f["cia/%s/old_wno" % table], f["cia/%s/log1e4" % table])
    return str(path)


def write_xsec(root, form):
    f = fixture()
    csv = {c: f["mol/csv/" + c] for c in ("pressure_bar", "temperature_K", "file_number", "number_wave_pts",
                                          "delta_wavenumber", "start_wavenumber")}
    gen.write_directory(str(root), form, csv, f["mol/rows"])
    return str(root)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def ulps(got, ref):
    """|got - ref| in units of the spacing of ``ref`` (0 where both are equal, NaNs included)."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    with np.errstate(all="ignore"):
        d = np.abs(got - ref) / np.spacing(np.abs(ref))
    return np.where(same, 0.0, d)
