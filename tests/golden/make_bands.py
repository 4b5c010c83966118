"""Generate tests/golden/bands.npz (build container only):

    python tests/golden/make_bands.py

The reference's ``retrieval`` module does not import here (ultranest, dynesty), so ``get_evaluations`` and
``get_chisq_max`` are taken from ``picaso/retrieval.py`` with ``ast`` and compiled at generation time, ``mean_regrid`` from
``picaso/justplotit.py``, ``create_grid`` from ``picaso/opacity_factory.py`` and ``chi_squared`` from
``picaso/analyze.py``; none of their text is stored.  ultranest's ``PredictionBand`` is stated by its published
definition: ``get_line(q) = scipy.stats.mstats.mquantiles(ys, q, axis=0)[0]``.  One statement is added to ``get_evaluations``: ``binning = False`` ahead of its body, without which its
``regrid=False`` path ends in a NameError.

The inputs are tests/bands_cases.py's (rebuilt by the tests from integer arithmetic); the file holds arrays only:
  M<S>/bands        (7, 33) mquantiles of fixture_matrix(S) at the seven levels, S in 1, 2, 3, 7, 64, 65, 1000
  M<S>/in_probe     every 5th value of the matrix
  E/<regrid>/spectra  (7, n) bands_spectra in KEYS order; /ptchem (3, 7, 20) bands_ptchem of temperature, H2O, CO2;
  E/<regrid>/max_logl_spectra, wavelength, err, offset; /chisq_* get_chisq_max's five results; regrid in newx, R, none
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bands_cases as bc            # noqa: E402

NAMES = ["temperature", "H2O", "CO2"]


class PredictionBand(object):
    """ultranest.plot.PredictionBand, as far as get_evaluations uses it."""

    def __init__(self, x):
        self.x = x
        self.ys = []

    def add(self, y):
        self.ys.append(y)

    def get_line(self, q=0.5):
        from scipy.stats.mstats import mquantiles
        return mquantiles(self.ys, q, axis=0)[0]


def _reference():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pandas as pd
    import ref_shim
    from scipy.stats import binned_statistic
    ns = {"np": np, "pd": pd, "binned_statistic": binned_statistic, "PredictionBand": PredictionBand}

    def take(fname, names, patch=None):
        path = os.path.join(ref_shim.REF_ROOT, "picaso", fname)
        with open(path) as fh:
            body = ast.parse(fh.read(), path).body
        nodes = [n for n in body if isinstance(n, ast.FunctionDef) and n.name in names]
        assert sorted(n.name for n in nodes) == sorted(names), (fname, names)
        if patch:
            patch(nodes)
        exec(compile(ast.fix_missing_locations(ast.Module(body=nodes, type_ignores=[])), path, "exec"), ns)

    def unbound(nodes):
        fn = [n for n in nodes if n.name == "get_evaluations"][0]
        fn.body.insert(1, ast.parse("binning = False").body[0])          # behind the docstring

    take("opacity_factory.py", ["create_grid"])
    take("justplotit.py", ["mean_regrid"])
    take("analyze.py", ["chi_squared"])
    take("retrieval.py", ["get_evaluations", "get_chisq_max"], patch=unbound)
    return ns


def main():
    from scipy.stats.mstats import mquantiles
    store = {}
    for S in bc.FIXTURE_DRAWS:
        y = bc.fixture_matrix(S)
        out = np.stack([np.asarray(mquantiles(y, q, axis=0)[0]) for q in bc.LEVELS])
        assert out.shape == (7, bc.FIXTURE_COLS)
        assert bc.same(out, bc.bands_numpy(y)), "the np.sort restatement differs from mquantiles at S = %d" % S
        store["M%d/bands" % S], store["M%d/in_probe" % S] = out, y.ravel()[::5]
        print("M%d: NaN lines in column 5: %d of 7" % (S, int(np.isnan(out[:, 5]).sum())))

    ns = _reference()
    samples = bc.toy_samples()
    best = samples[17]
    for name, regrid in bc.toy_regrids().items():
        np.random.seed(bc.SEED_E)
        ev = ns["get_evaluations"](samples, best, bc.toy_model(frame=True), bc.NDRAWS_E, regrid=regrid,
                                   pressure_bands=NAMES)
        key = "E/%s/" % name
        store[key + "spectra"] = np.stack([np.asarray(ev["bands_spectra"][k]) for k in bc.KEYS])
        store[key + "ptchem"] = np.stack([[np.asarray(ev["bands_ptchem"][n][k]) for k in bc.KEYS] for n in NAMES])
        store[key + "max_logl_spectra"] = np.asarray(ev["max_logl_spectra"])
        store[key + "wavelength"] = np.asarray(ev["wavelength"])
        store[key + "err"] = np.asarray(ev["max_logl_error_inflation"])
        store[key + "offset"] = np.asarray(ev["max_logl_offsets"]["nirspec"])
        store[key + "pressure"] = np.asarray(ev["pressure"])
        chi = ns["get_chisq_max"](ev, bc.toy_data())
        for k, v in chi.items():
            store[key + "chisq_" + k] = np.asarray(v)
        print(key, store[key + "spectra"].shape, "chisq per data point %.6g" % chi["chisq_per_datapt"])
    store["E/in_probe"] = np.concatenate([samples.ravel()[::7], best])

    path = os.path.join(HERE, "bands.npz")
    np.savez_compressed(path, **store)
    size = os.path.getsize(path)
    print("wrote", path, "%.1f KB" % (size / 1024))
    assert size <= 400 * 1024, "the fixture is meant to stay small"


if __name__ == "__main__":
    main()
