"""The inputs of tests/golden/bands.npz and the numpy restatement of a prediction band, shared by the fixture's generator
(tests/golden/make_bands.py) and the tests (test_bands_host.py, test_bands_gpu.py).  The inputs come from integer-hash
arithmetic and correctly rounded operations (gridfit_cases.hash01), so every machine rebuilds the same bits.

  M<S>    S in FIXTURE_DRAWS draws x 33 columns: magnitudes over 2^-40 .. 2^40 with both signs, column 5 holds one NaN,
          column 7 is constant, column 9 holds ties
  E       the get_evaluations case: a toy model of six parameters, 200 posterior samples, 64 draws, profiles of 20 levels
"""
import numpy as np

from gridfit_cases import hash01

FIXTURE_DRAWS = (1, 2, 3, 7, 64, 65, 1000)
FIXTURE_COLS = 33
# the reference's seven levels in its own expressions (retrieval.py:288-296), in its order of keys
KEYS = ("1sig_lo", "1sig_hi", "2sig_lo", "2sig_hi", "3sig_lo", "3sig_hi", "median")
LEVELS = []
for _q in [k / 100 / 2 for k in [68.27, 95.45, 99.73]]:
    LEVELS += [0.5 - _q, 0.5 + _q]
LEVELS += [0.5]


# ---------------------------------------------------------------------------------------------- the restatement
def table_numpy(n, q, alphap=0.4, betap=0.4):
    """scipy's ``_quantiles1D`` table for ``n >= 2`` sorted values: ``(k, gamma)``."""
    p = np.atleast_1d(np.asarray(q, dtype=float))
    m = alphap + p * (1. - alphap - betap)
    aleph = (n * p + m)
    k = np.floor(aleph.clip(1, n - 1)).astype(int)
    gamma = (aleph - k).clip(0, 1)
    return k, gamma


def lines_numpy(ys, k, gamma):
    """The lines ``(k, gamma)`` of every column of ``ys`` (S, N) on ``np.sort``: ``mquantiles(ys, q, axis=0)`` for the
    table of ``q``, (len(k), N)."""
    x = np.sort(np.asarray(ys, dtype=float), axis=0)
    k, gamma = np.asarray(k), np.asarray(gamma, dtype=float)
    if x.shape[0] == 1:
        return np.repeat(x, len(k), axis=0)
    with np.errstate(all="ignore"):
        return (1. - gamma)[:, None] * x[k - 1] + gamma[:, None] * x[k]


def bands_numpy(ys, q=LEVELS):
    ys = np.asarray(ys, dtype=float)
    if ys.shape[0] == 1:
        return np.repeat(ys, len(np.atleast_1d(q)), axis=0)
    return lines_numpy(ys, *table_numpy(ys.shape[0], q))


def same(a, b):
    """Equal by value, NaN in the same places (``-0.0 == +0.0``)."""
    return np.array_equal(a, b, equal_nan=True)


# ---------------------------------------------------------------------------------------------- inputs
def matrix(S, N=FIXTURE_COLS, seed=0):
    """(S, N) draws: signs mixed, magnitudes 2^-40 .. 2^40 changing from column to column."""
    u = hash01(S * N, 9000 + 131 * seed + S).reshape(S, N)
    sgn = np.where(hash01(S * N, 77 + seed + S).reshape(S, N) < 0.4, -1.0, 1.0)
    expo = ((np.arange(N) * 37) % 81 - 40).astype(np.int32)
    return sgn * np.ldexp(0.5 + u, expo[None, :])


def fixture_matrix(S):
    y = matrix(S)
    y[:, 7] = 0.375
    y[:, 9] = np.floor(y[:, 9] * 4.0) / 4.0 if S < 8 else np.floor(hash01(S, 5) * 5.0)
    y[S // 2, 5] = np.nan
    return y


NSAMPLES_E, NDRAWS_E, NLEVEL_E, NWNO_E, SEED_E = 200, 64, 20, 1500, 1234


class ToyInputs:
    """What ``model(..., return_ptchem=True)`` returns: an object with ``inputs['atmosphere']['profile']``."""

    def __init__(self, profile):
        self.inputs = {"atmosphere": {"profile": profile}}


def toy_samples():
    lo = np.array([0.010, -1.0, 800.0, 1.0, -2.0, 0.0])
    hi = np.array([0.012, 1.0, 1200.0, 5.0, 2.0, 1e-9])
    return lo + hash01(NSAMPLES_E * 6, 4242).reshape(NSAMPLES_E, 6) * (hi - lo)


def toy_model(frame=False, as_dict=False):
    """``model(params, return_ptchem=False)`` of six parameters: a spectrum on 1 500 increasing wavenumbers from products
    and sums alone, an offset for the data set 'nirspec', an error inflation, and a profile of 20 levels -- a dictionary of
    columns, or a DataFrame (``frame``), on the inputs object or in a one-entry dictionary of them (``as_dict``)."""
    wno = 2004.0 + 4.0 * np.arange(NWNO_E)                  # 1.25 .. 4.99 micron; 1e4 / (1e4 / 8000.) is 8000. again
    t = 1e4 / wno - 3.0
    lev = np.arange(NLEVEL_E) / float(NLEVEL_E)
    pressure = np.ldexp(1.0, np.arange(NLEVEL_E) - 14)

    def model(params, return_ptchem=False):
        p = np.asarray(params, dtype=float)
        if return_ptchem:
            prof = {"pressure": pressure, "temperature": p[2] * (0.6 + 0.8 * lev * lev),
                    "H2O": 1e-4 * p[3] * (1.0 + 0.5 * lev), "CO2": 1e-6 * p[3] * p[3] * (1.5 - lev)}
            if frame:
                import pandas as pd
                prof = pd.DataFrame(prof)
            obj = ToyInputs(prof)
            return {"opa db1": obj} if as_dict else obj
        y = p[0] + 0.0005 * p[1] * t * (1.0 - 0.3 * t * t) + 1e-6 * p[3] * t * t
        return wno, y, {"nirspec": 1e-5 * p[4]}, p[5]
    return model


def toy_regrids():
    """``regrid`` of the three fixture cases: a wavenumber array, a float resolution, ``False``."""
    return {"newx": 2100.0 + 61.0 * np.arange(90), "R": 80.0, "none": False}


def toy_data():
    """``data_dict`` of get_chisq_max: two data sets ``(wavenumber, y, e)``, one of them with an offset of its own."""
    x1, x2 = 2300.0 + 150.0 * np.arange(20), 5400.0 + 170.0 * np.arange(14)
    return {"nirspec": (x1, 0.011 + 0.0002 * (hash01(20, 61) - 0.5), 0.0001 * (0.5 + hash01(20, 62))),
            "miri": (x2, 0.011 + 0.0002 * (hash01(14, 63) - 0.5), 0.0001 * (0.5 + hash01(14, 64)))}
