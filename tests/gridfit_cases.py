"""The inputs of tests/golden/gridfit.npz, shared by its generator (tests/golden/make_gridfit.py) and the tests
(test_gridfit_host.py, test_gridfit_gpu.py).  Everything comes from integer-hash arithmetic, exact powers of two and
correctly rounded operations, so every machine rebuilds the same bits; the fixture holds a probe of them.

  I1..I5  d = 1..5 parameters, 2-4 nodes each, models in shuffled order, nwave = 4099 (no multiple of 64), magnitudes from
          2^-60 to 2^60 along a row with both signs, 40 goals: all parameters on the last node, on the first node, above
          the last node, on an inner node, then mixtures of these with values inside the grid
  I6      3 x 3 nodes, the centre model absent: every cell touches the hole, every goal takes the fallback
  F1      24 models (3 x 4 x 2), nwave = 4096, 60 data points whose bins hold 0, 1, 63, 64, 65 and > 1024 columns, columns
          outside every bin.  An empty bin makes every chi squared NaN (in the reference as here), so the data set
          'F1' carries the comparison of the binned models, and 'F1b' -- the same centres without those of the empty
          bins -- the offsets, chi squares, ranks and posteriors
  F2      F1 with the wavelength array (and the spectra) in decreasing order
  L1      200 goals on F1's grid against F1b's data with per-sample offset, scaling and err_inf
"""
import itertools

import numpy as np

NAMES = ("mh", "cto", "tint", "logkzz", "fsed")          # the first four are planet_params, the last a cld_params
NODES = {1: (4,), 2: (3, 4), 3: (2, 3, 4), 4: (2, 3, 2, 3), 5: (2, 3, 2, 2, 3)}
NODE_VALUES = ((-1.0, -0.3, 0.5, 1.7), (0.25, 0.458, 0.55, 0.916), (100.0, 200.0, 300.7, 450.1), (7.0, 9.1, 10.2, 11.0),
               (0.3, 1.0, 3.3, 10.0))
NWAVE_I, NGOALS_I = 4099, 40
PROBE = 17                                               # the fixture keeps every 17th column and a digest of all


def hash01(n, seed):
    """``n`` doubles in [0, 1) from a 64-bit integer mix of the index (wrapping uint64 arithmetic: exact everywhere)."""
    with np.errstate(over="ignore"):
        h = (np.arange(n, dtype=np.uint64) + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
        h ^= h >> np.uint64(29)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(32)
    return (h >> np.uint64(11)).astype(np.float64) / 9007199254740992.0


def digest(a):
    """(rows, 2) uint64 of a 2-D float64 array: the xor and the wrapping sum of every row's bit patterns -- equal digests
    and equal probe columns stand for ``np.array_equal`` of arrays the fixture cannot hold (1 MiB)."""
    b = np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    with np.errstate(over="ignore"):
        return np.stack([np.bitwise_xor.reduce(b, axis=1), np.add.reduce(b, axis=1, dtype=np.uint64)], axis=1)


def _params(cols):
    """``grid_params`` in the reference's layout from the (nmodels, d) table of values."""
    gp = {"planet_params": {}}
    for p in range(cols.shape[1]):
        group = "cld_params" if NAMES[p] == "fsed" else "planet_params"
        gp.setdefault(group, {})[NAMES[p]] = cols[:, p].copy()
    return gp


def _square(counts, seed, drop=()):
    """Every combination of the first ``counts[p]`` node values of parameter ``p``, shuffled; ``drop``: combinations
    (index tuples) left out."""
    combos = [c for c in itertools.product(*[range(n) for n in counts]) if c not in drop]
    order = np.argsort(hash01(len(combos), seed), kind="stable")
    idx = np.array(combos)[order]
    return np.stack([np.array(NODE_VALUES[p])[idx[:, p]] for p in range(len(counts))], axis=1)


def _steep_rows(nmodels, nwave, seed):
    """Rows whose magnitudes run from 2^-60 to 2^60 along the row, a third of the values negative."""
    i = np.arange(nwave)
    expo = (i * 121 // nwave - 60).astype(np.int32)
    out = np.empty((nmodels, nwave))
    for m in range(nmodels):
        u, sgn = hash01(nwave, seed + 7919 * m), hash01(nwave, seed + 7919 * m + 3)
        out[m] = np.where(sgn < 1.0 / 3.0, -1.0, 1.0) * np.ldexp(0.5 + u, expo)
    return out


def interp_case(d):
    """I<d>: ``(wavelength, spectra, grid_params, goals (40, d))``."""
    counts = NODES[d]
    cols = _square(counts, 100 + d)
    wl = np.linspace(0.6, 5.3, NWAVE_I)
    spectra = _steep_rows(cols.shape[0], NWAVE_I, 1000 * d)
    goals = np.empty((NGOALS_I, d))
    for p in range(d):
        arr = np.array(NODE_VALUES[p][:counts[p]])
        first, last, prev = arr[0], arr[-1], arr[-2]
        above = last + 0.37 * (last - prev)
        inner = arr[1] if counts[p] > 2 else arr[0]
        u, pick = hash01(NGOALS_I, 50 * d + p), hash01(NGOALS_I, 50 * d + p + 25)
        inside = first + u * (last - first)
        mixed = np.where(pick < 0.1, last, np.where(pick < 0.2, first, np.where(pick < 0.3, above,
                                                                                  np.where(pick < 0.4, inner, inside))))
        goals[:, p] = mixed
        goals[0, p], goals[1, p], goals[2, p], goals[3, p] = last, first, above, inner
    return wl, spectra, _params(cols), goals


def hole_case():
    """I6: ``(wavelength, spectra, grid_params, goals (12, 2))``; goal 11 sits exactly on an existing model (NaN)."""
    cols = _square((3, 3), 106, drop=((1, 1),))
    nwave = 257
    wl = np.linspace(0.6, 5.3, nwave)
    spectra = _steep_rows(cols.shape[0], nwave, 6000)
    a, b = np.array(NODE_VALUES[0][:3]), np.array(NODE_VALUES[1][:3])
    fa = np.array([0.11, 0.83, 0.47, 0.29, 0.62, 0.93, 0.05, 0.71, 0.38, 0.56, 1.21])
    fb = np.array([0.74, 0.19, 0.58, 0.91, 0.33, 0.08, 0.66, 0.97, 0.23, 0.41, 0.52])
    goals = np.empty((12, 2))
    goals[:11, 0] = a[0] + fa * (a[2] - a[0])
    goals[:11, 1] = b[0] + fb * (b[2] - b[0])
    goals[11] = (a[1], b[0])
    return wl, spectra, _params(cols), goals


NWAVE_F = 4096


def _wiggle(wl):
    """A spectral feature from products and sums alone (no libm: the same bits everywhere)."""
    t = wl - 3.0
    return t * (1.0 - 0.3 * t * t) * (1.0 + 0.5 * t)


def fit_case(decreasing=False):
    """F1 (F2: ``decreasing``): ``(wavelength, spectra (24, 4096), grid_params)``."""
    cols = _square((3, 4, 2), 201)
    wl = 1.0 + np.arange(NWAVE_F) / 1024.0                       # exact: 1 ... 4.999
    n = cols.shape[0]
    spectra = np.empty((n, NWAVE_F))
    for m in range(n):
        mh, cto, tint = cols[m]
        spectra[m] = (0.0100 + 0.0004 * mh + 0.0010 * cto * _wiggle(wl) + 0.000002 * tint * (wl - 3.0)
                      + 0.00002 * (hash01(NWAVE_F, 300 + m) - 0.5))
    if decreasing:
        wl, spectra = wl[::-1].copy(), np.ascontiguousarray(spectra[:, ::-1])
    return wl, spectra, _params(cols)


def fit_data(name):
    """``(wlgrid_center, wlgrid_width, y_data, e_data)`` of 'F1' (60 points, empty bins among them) or 'F1b' (without
    the centres of the empty bins).  The centres are placed in units of the grid's spacing, 1 / 1024: runs of constant
    spacing s give bins of exactly s columns."""
    steps = ([64] * 3 + [63] * 3 + [65] * 3 + [1] * 4 + [0.25] * 6 + [40.5] * 3 + [1100] * 2 + [7] * 10 + [3.5] * 12
             + [120] * 5 + [17] * 8)
    pos = 200.5 + np.concatenate(([0.0], np.cumsum(steps)))
    assert pos.size == 60 and pos[-1] < NWAVE_F - 100
    centres = 1.0 + pos / 1024.0
    if name == "F1b":
        edges = np.concatenate(([pos[0] - steps[0] / 2], (pos[:-1] + pos[1:]) / 2, [pos[-1] + steps[-1] / 2]))
        count = np.diff(np.ceil(edges))
        centres = centres[count > 0]
    elif name != "F1":
        raise KeyError(name)
    n = centres.size
    y = (0.0100 + 0.0004 * 0.1 + 0.0010 * 0.5 * _wiggle(centres) + 0.000002 * 260.0 * (centres - 3.0) + 0.0007
         + 0.00008 * (hash01(n, 401) - 0.5))
    e = 0.00004 * (0.5 + hash01(n, 402))
    return centres, np.gradient(centres), y, e


NGOALS_L = 200


def loglike_case():
    """L1: ``(goals (200, 3), offset, scaling, err_inf)`` on F1's grid."""
    goals = np.empty((NGOALS_L, 3))
    for p, n in enumerate((3, 4, 2)):
        arr = np.array(NODE_VALUES[p][:n])
        goals[:, p] = arr[0] + hash01(NGOALS_L, 500 + p) * (arr[-1] - arr[0]) * 1.04
    goals[0] = [NODE_VALUES[0][2], NODE_VALUES[1][3], NODE_VALUES[2][1]]
    goals[1] = [NODE_VALUES[0][0], NODE_VALUES[1][0], NODE_VALUES[2][0]]
    offset = 0.0002 * (hash01(NGOALS_L, 510) - 0.5)
    scaling = 0.9 + 0.2 * hash01(NGOALS_L, 511)
    err_inf = 1e-9 * hash01(NGOALS_L, 512)
    return goals, offset, scaling, err_inf


def add_case(fitter, grid_name, case):
    wl, spectra, gp = case[:3]
    fitter.add_grid(grid_name, wl, spectra, gp)
    return fitter


def eval_tables(spectra, rows, wts, kcount, div):
    """The formula of picaso_grid_rows_dev in numpy: per sample (((0.0 + w0 g[r0]) + w1 g[r1]) + ...) / div."""
    out = np.empty((rows.shape[0], spectra.shape[1]))
    with np.errstate(all="ignore"):
        for s in range(rows.shape[0]):
            v = np.zeros(spectra.shape[1])
            for c in range(kcount[s]):
                v = v + wts[s, c] * spectra[rows[s, c]]
            out[s] = v / div[s]
    return out
