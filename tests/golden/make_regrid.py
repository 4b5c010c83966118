"""Generate tests/golden/regrid.npz by running the REFERENCE's own ``mean_regrid`` and ``create_grid`` (build container only):

    python tests/golden/make_regrid.py

The reference's plotting module does not import as a whole without a plotting library, so the two function definitions
are taken from their files with ``ast`` and compiled at generation time next to ``scipy.stats.binned_statistic``; none
of their text is stored.  Arrays only: per case ``<case>/centres`` (what ``mean_regrid`` returns first), ``<case>/expected``
(6, nbins) (what it returns second, per row), ``<case>/counts`` (``np.histogram`` of the grid over the same edges),
``<case>/edges`` and ``<case>/y_probe`` (every 97th column of the inputs: the inputs themselves are rebuilt by ``case()``
below, by the generator and the tests alike, from integer arithmetic and exact powers of two -- the same bits on every
machine -- so the file stays a few tens of kB).

Cases (six ``y`` rows each):
  A  x = linspace(2000, 33333, 4096), R = 100: bins of 2 to ~45 points
  B  x = linspace(2000, 33333, 8192), newx of 5 coarse points well inside the range: bins of well over 1 024 points, columns
     outside both ends
  C  x as in A with a gap cut out, newx finer than x over part of the range: empty bins (NaN) and one-point bins
  D  x = arange(0, 40, 0.5), newx = [10.5, 20.5, 30.5]: edges 5.5 / 15.5 / 25.5 / 35.5, columns on every edge, the closed
     last one included, and beyond both ends
  E  newx of two points
  F  rows whose magnitudes span 2^-100 ... 2^100 (1e-30 ... 1e30) within one bin, so that the order of summation shows;
     the last row carries a NaN and an inf in one bin.  scipy's binned_statistic refuses non-finite values, so THAT row's
     expectation is ``np.bincount(idx, weights) / counts`` with the bin numbers binned_statistic assigns -- the very
     expression it evaluates for the finite rows (asserted here against the reference for every finite row).
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CASES = ("A", "B", "C", "D", "E", "F")
NROWS = 6


def _hash01(n, seed):
    """``n`` doubles in [0, 1) from a 64-bit integer mix of the index (wrapping uint64 arithmetic: exact everywhere)."""
    with np.errstate(over="ignore"):
        h = (np.arange(n, dtype=np.uint64) + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
        h ^= h >> np.uint64(29)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(32)
    return (h >> np.uint64(11)).astype(np.float64) / 9007199254740992.0


def _rows(n, seed, span):
    """Six rows of ``n`` values: positive and smooth-ish, signed, steep (``span`` binary orders of magnitude along the
    row), cancelling pairs, zeros of both signs with subnormals, and magnitudes scattered over +-``span`` orders."""
    u = [_hash01(n, seed + 1000 * r) for r in range(8)]
    i = np.arange(n)
    y = np.empty((NROWS, n))
    y[0] = 0.25 + 0.5 * u[0]
    y[1] = u[1] - 0.5
    y[2] = np.ldexp(0.5 + u[2], -(i * span // max(n, 1)).astype(np.int32))
    y[3] = np.where(i % 2 == 0, 1.0, -1.0) * np.ldexp(1.0 + u[3], 40) + u[4]
    y[4] = np.where(u[5] < 0.3, -0.0, np.where(u[5] < 0.6, 0.0, np.ldexp(u[6], -1060)))
    y[5] = (u[7] - 0.5) * np.ldexp(1.0, (np.floor(u[0] * (2 * span + 1)) - span).astype(np.int32))
    return y


def case(name):
    """``(x, y (6, n), newx | None, R | None)`` of one case."""
    if name == "A":
        x = np.linspace(2000.0, 33333.0, 4096)
        return x, _rows(x.size, 11, 60), None, 100
    if name == "B":
        x = np.linspace(2000.0, 33333.0, 8192)
        return x, _rows(x.size, 12, 60), np.array([6000.0, 10000.0, 14000.0, 19000.0, 24000.0]), None
    if name == "C":
        x = np.linspace(2000.0, 33333.0, 4096)
        x = x[(x < 9000.0) | (x > 12000.0)]
        newx = np.concatenate([np.linspace(3000.0, 8000.0, 40), np.linspace(8200.0, 14000.0, 2001)[1:],
                               np.linspace(14500.0, 30000.0, 25)])
        return x, _rows(x.size, 13, 60), newx, None
    if name == "D":
        x = np.arange(0.0, 40.0, 0.5)
        return x, _rows(x.size, 14, 20), np.array([10.5, 20.5, 30.5]), None
    if name == "E":
        x = np.linspace(2000.0, 33333.0, 777)
        return x, _rows(x.size, 15, 60), np.array([9000.0, 21000.0]), None
    if name == "F":
        x = np.linspace(2000.0, 33333.0, 1500)
        y = _rows(x.size, 16, 100)
        y[:5] = y[5] * np.ldexp(1.0, np.arange(5, dtype=np.int32) - 2)[:, None] * (1.0 + 0.25 * _rows(x.size, 17, 100)[0])
        y[5, 700] = np.nan
        y[5, 705] = np.inf
        y[5, 40] = -np.inf
        return x, y, np.linspace(4000.0, 30000.0, 9), None
    raise KeyError(name)


def _reference_functions():
    """``mean_regrid`` (justplotit.py) and ``create_grid`` (opacity_factory.py) compiled from the reference tree."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ref_shim
    from scipy.stats import binned_statistic
    ns = {"np": np, "binned_statistic": binned_statistic}
    for fname, func in (("opacity_factory.py", "create_grid"), ("justplotit.py", "mean_regrid")):
        path = os.path.join(ref_shim.REF_ROOT, "picaso", fname)
        with open(path) as fh:
            tree = ast.parse(fh.read(), path)
        node = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == func]
        assert len(node) == 1, (fname, func)
        exec(compile(ast.Module(body=node, type_ignores=[]), path, "exec"), ns)
    return ns["mean_regrid"], ns["create_grid"]


def main():
    mean_regrid, create_grid = _reference_functions()
    store = {}
    for name in CASES:
        x, y, newx, R = case(name)
        if R is not None:
            edges = np.asarray(create_grid(1e4 / max(x), 1e4 / min(x), R), dtype=float)
        else:
            d = np.diff(newx)
            edges = np.concatenate(([newx[0] - d[0] / 2], newx[:-1] + d / 2.0, [newx[-1] + d[-1] / 2]))
        counts = np.histogram(x, bins=edges)[0]
        nb = edges.size - 1
        idx = np.searchsorted(edges, x, side="right") - 1
        idx[x == edges[-1]] = nb - 1
        ok = (idx >= 0) & (idx < nb)
        expected = np.empty((NROWS, nb))
        centres = None
        for r in range(NROWS):
            with np.errstate(all="ignore"):
                by_count = np.where(counts > 0, np.bincount(idx[ok], weights=y[r][ok], minlength=nb) / counts, np.nan)
            if np.all(np.isfinite(y[r])):
                centres, expected[r] = mean_regrid(x, y[r], newx=newx, R=R)
                assert np.array_equal(expected[r], by_count, equal_nan=True), (name, r)
            else:
                assert name == "F" and r == 5
                expected[r] = by_count
        assert np.array_equal(np.bincount(idx[ok], minlength=nb), counts)
        store[name + "/centres"], store[name + "/expected"] = np.asarray(centres), expected
        store[name + "/counts"], store[name + "/edges"] = counts, edges
        store[name + "/y_probe"] = y[:, ::97]
        print(name, "n = %d, nbins = %d, counts %d..%d, empty %d" % (x.size, nb, counts.min(), counts.max(), (counts == 0).sum()))
    path = os.path.join(HERE, "regrid.npz")
    np.savez_compressed(path, **store)
    size = os.path.getsize(path)
    print("wrote", path, "%.1f KB" % (size / 1024))
    assert size <= 1024 * 1024, "a committed file holds 1 MiB"


if __name__ == "__main__":
    main()
