"""Generate tests/golden/convolve.npz by running the REFERENCE's own ``conv_non_uniform_R`` (build container only):

    python tests/golden/make_convolve.py

The reference's retrieval driver does not import as a whole without its samplers, so the function definition is taken from
driver.py with ``ast`` and compiled at generation time; none of its text is stored.  Arrays only: per case
``<case>/expected`` (2, nobs) (the function's result for the positive and the signed row), ``<case>/expected_abs`` (2, nobs)
(its result for the rows' absolute values: the scale of the tolerance), ``<case>/wl``, ``<case>/R`` and ``<case>/y_probe``
(every 97th column of the rows).  The inputs themselves are rebuilt by ``case()`` below, by the generator and the tests
alike, from integer arithmetic (``make_regrid._rows`` / ``_hash01``), so the file stays a few kB.

Cases (x: wavenumbers, the model wavelengths are 1e4 / x; data points in um):
  A  x = linspace(2000, 33333, 4096); 37 points over 0.35-4.9 um, R = 100 varying +-30 % from point to point: windows up to
     ~1 150 columns
  B  x = linspace(2000, 33333, 8192); 50 points, R = 1000 +-10 %: windows of some 15 to 250 columns, under one workgroup's
     width, several shorter than one wave
  C  x as in A; 12 points at R = 30 +-10 %: a window covering most of the grid; points in descending order, one of them
     given twice
  D  x as in A; three points inside the grid, one more than 39 sigma beyond each end of it (NaN: no weight at all)
  E  80 columns at 1.80, 1.79, ... 1.01 um; windows of 0, 1, 2, 63, 64 and 65 columns by choice of R (the empty one lies
     between two columns: NaN)
No point lies between 30 and 39 sigma outside the grid, where both of the reference's sums are subnormal.
"""
import ast
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CASES = ("A", "B", "C", "D", "E")
ROWS = (0, 1)             # of make_regrid._rows: the positive row and the signed row

_spec = importlib.util.spec_from_file_location("make_regrid", os.path.join(HERE, "make_regrid.py"))
make_regrid = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_regrid)


def _spread(n, seed, width):
    """``n`` factors in [1 - width, 1 + width)"""
    return 1.0 + width * (2.0 * make_regrid._hash01(n, seed) - 1.0)


def case(name):
    """``(x, y (2, n), wl, R)`` of one case."""
    if name in ("A", "C", "D"):
        x = np.linspace(2000.0, 33333.0, 4096)
    elif name == "B":
        x = np.linspace(2000.0, 33333.0, 8192)
    elif name == "E":
        x = 1e4 / ((180 - np.arange(80)) / 100.0)
    else:
        raise KeyError(name)
    y = make_regrid._rows(x.size, 20 + CASES.index(name), 60)[list(ROWS)]
    if name == "A":
        wl = 0.35 + (4.9 - 0.35) * np.arange(37) / 36.0
        R = 100.0 * _spread(37, 501, 0.3)
    elif name == "B":
        wl = 0.35 + (4.9 - 0.35) * np.arange(50) / 49.0
        R = 1000.0 * _spread(50, 502, 0.1)
    elif name == "C":
        wl = 4.6 - 0.38 * np.arange(12)
        wl[7] = wl[3]
        R = 30.0 * _spread(12, 503, 0.1)
        R[7] = R[3]
    elif name == "D":
        wl = np.array([7.0, 0.4, 2.2, 4.85, 0.2])
        R = np.full(5, 100.0)
    else:
        centre = np.array([1.405, 1.40, 1.405, 1.40, 1.405, 1.40])
        half = np.array([0.002, 0.004, 0.008, 0.314, 0.318, 0.324])          # 39 sigma: 0, 1, 2, 63, 64, 65 columns
        wl, R = centre, 39.0 * centre / (2.355 * half)
    return x, y, wl, R


def _reference_function():
    """``conv_non_uniform_R`` compiled from the reference tree's driver.py."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ref_shim
    path = os.path.join(ref_shim.REF_ROOT, "picaso", "driver.py")
    with open(path) as fh:
        tree = ast.parse(fh.read(), path)
    node = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "conv_non_uniform_R"]
    assert len(node) == 1
    ns = {"np": np}
    exec(compile(ast.Module(body=node, type_ignores=[]), path, "exec"), ns)
    return ns["conv_non_uniform_R"]


def main():
    conv = _reference_function()
    store = {}
    for name in CASES:
        x, y, wl, R = case(name)
        model_wl = 1e4 / x
        with np.errstate(all="ignore"):
            expected = np.stack([conv(row, model_wl, R, wl) for row in y])
            expected_abs = np.stack([conv(np.abs(row), model_wl, R, wl) for row in y])
        store[name + "/expected"], store[name + "/expected_abs"] = expected, expected_abs
        store[name + "/wl"], store[name + "/R"] = wl, R
        store[name + "/y_probe"] = y[:, ::97]
        print(name, "n = %d, nobs = %d, NaN %d" % (x.size, wl.size, int(np.isnan(expected[0]).sum())))
    path = os.path.join(HERE, "convolve.npz")
    np.savez_compressed(path, **store)
    size = os.path.getsize(path)
    print("wrote", path, "%.1f KB" % (size / 1024))
    assert size <= 1024 * 1024, "a committed file holds 1 MiB"


if __name__ == "__main__":
    main()
