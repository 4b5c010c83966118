"""Generate tests/golden/retrieve.npz by running the REFERENCE's own retrieval driver functions (build container only):

    python tests/golden/make_retrieve.py

The reference's ``driver`` module does not import here (astropy, dynesty, mpi4py), so ``prior_finder``, ``hypercube``,
``set_dict_value``, ``find_values_for_key`` and ``log_likelihood`` are taken from ``picaso/driver.py`` with ``ast`` and
compiled at generation time next to numpy and scipy; none of their text is stored.  ``MODEL`` in that namespace is a stub
that returns stored arrays: the likelihood is checked for the reference's arithmetic given a model, not for the model.

The file holds inputs and outputs only:
  meta/numpy, meta/scipy        the versions that wrote it
  config                        JSON: the ``retrieval`` section (nested priors: uniform, gaussian and ``log`` ones, a
                                ``sampler`` block without priors, offset / scaling / err_inf entries for two instruments)
  prior_keys                    JSON: the keys of prior_finder(config), in order
  cube/u, cube/x                7 unit-cube points (0.5, values near 0 and 1 among them) and hypercube of each
  setdict                       JSON: [[path, value, returned, dictionary afterwards]]
  findvalues                    JSON: [[dictionary, key, result]]
  ll/cases                      JSON: [{name, N, retrieval (which of offset / scaling / err_inf the configuration has)}]
  ll/data/<inst>/x, y, e        the two data sets (5 and 3 points)
  ll/<name>/cube, model/<inst>  the cube of a case and the model MODEL's stub returned, (N, ndata)
  ll/<name>/out                 what log_likelihood returned: () for N = 1, (N,) otherwise
"""
import ast
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

NAMES = ["prior_finder", "hypercube", "set_dict_value", "find_values_for_key", "log_likelihood"]
INSTRUMENTS = ("nirspec", "miri")

RETRIEVAL = {
    "temperature": {"knots": {"T_knots": {
        "k1": {"prior": "uniform", "log": False, "uniform_kwargs": {"min": 300.0, "max": 2500.0}},
        "k2": {"prior": "gaussian", "log": False, "gaussian_kwargs": {"mean": 1200.0, "std": 150.0}}}}},
    "chemistry": {"free": {
        "H2O": {"prior": "uniform", "log": True, "uniform_kwargs": {"min": -9.0, "max": -1.5}},
        "CH4": {"prior": "gaussian", "log": True, "gaussian_kwargs": {"mean": -4.0, "std": 0.7}}}},
    "sampler": {"resume": False, "sampler_kwargs": {"nlive": 50}, "run_kwargs": {"dlogz_init": 0.5}},
    "offset": {"miri": {"prior": "uniform", "log": False, "uniform_kwargs": {"min": -1e-16, "max": 1e-16}}},
    "scaling": {"nirspec": {"prior": "uniform", "log": False, "uniform_kwargs": {"min": 0.5, "max": 1.5}}},
    "err_inf": {"miri": {"prior": "uniform", "log": True, "uniform_kwargs": {"min": -34.0, "max": -30.0}},
                "nirspec": {"prior": "uniform", "log": True, "uniform_kwargs": {"min": -34.0, "max": -30.0}}},
}


def _reference():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ref_shim
    from collections.abc import Mapping
    from scipy import stats
    ns = {"np": np, "stats": stats, "Mapping": Mapping}
    path = os.path.join(ref_shim.REF_ROOT, "picaso", "driver.py")
    with open(path) as fh:
        body = ast.parse(fh.read(), path).body
    nodes = [n for n in body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert sorted(n.name for n in nodes) == sorted(NAMES)
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
    return ns


def main():
    import scipy
    ns = _reference()
    store = {"meta/numpy": np.array(np.__version__), "meta/scipy": np.array(scipy.__version__)}
    store["config"] = np.array(json.dumps(RETRIEVAL))
    fitpars = ns["prior_finder"](RETRIEVAL)
    store["prior_keys"] = np.array(json.dumps(list(fitpars.keys())))
    ndim = len(fitpars)

    rng = np.random.default_rng(20261021)
    u = rng.random((7, ndim))
    u[0] = 0.5
    u[1] = 1e-12
    u[2] = 1.0 - 1e-12
    u[3, ::2] = 2.0 ** -30
    store["cube/u"] = u
    store["cube/x"] = np.array([ns["hypercube"](row, fitpars) for row in u])

    nested = {"a": {"b": {"value": 1.0, "unit": "bar"}, "c": 3}, "d": {"value": 2.0}}
    rows = []
    for path_string, value in (("a.b.value", 7.5), ("d.value", -1.0), ("a.c", 4), ("a.x.value", 1.0), ("a.b.nothere", 2.0),
                               ("a.c.value", 1.0)):
        data = copy.deepcopy(nested)
        rows.append([path_string, value, bool(ns["set_dict_value"](data, path_string, value)), data])
    store["setdict"] = np.array(json.dumps(rows))

    crawl = {"clouds": {"c1_type": "brewster_mie", "c1": {"brewster_mie": {"condensate": "SiO2"}},
                        "c2": {"flex_fsed": {"condensate": ["MgSiO3", "SiO2"]}}},
             "list": [{"condensate": "Fe"}, 3], "other": {"x": 1}}
    store["findvalues"] = np.array(json.dumps([[crawl, key, ns["find_values_for_key"](crawl, key)]
                                               for key in ("condensate", "x", "absent")]))

    # ---- log_likelihood: MODEL is a stub that returns the stored arrays
    data = {"nirspec": [np.linspace(2000.0, 3300.0, 5), 1e-15 * (1.0 + 0.3 * np.cos(np.arange(5.0))), 1e-16 * (1.0 + 0.1 * np.arange(5.0))],
            "miri": [np.linspace(900.0, 1500.0, 3), 3e-16 * (1.0 + 0.2 * np.sin(np.arange(3.0))), np.full(3, 4e-17)]}
    for key, (x, y, e) in data.items():
        store["ll/data/%s/x" % key], store["ll/data/%s/y" % key], store["ll/data/%s/e" % key] = x, y, e
    config_base = {"InputOutput": {"observation_data": {k: "unused" for k in INSTRUMENTS}}}
    cases = []
    variants = {"all": ("offset", "scaling", "err_inf"), "none": (), "offset": ("offset",), "scaling": ("scaling",),
                "err_inf": ("err_inf",)}
    for vname, present in variants.items():
        for N in (1, 3):
            name = "%s_N%d" % (vname, N)
            retrieval = {k: v for k, v in RETRIEVAL.items() if k not in ("offset", "scaling", "err_inf") or k in present}
            config = dict(config_base, retrieval=retrieval)
            fp = ns["prior_finder"](retrieval)
            cube = np.array([ns["hypercube"](row, fp) for row in rng.random((N, len(fp)))])
            model = {k: data[k][1][None, :] * (1.0 + 0.05 * rng.standard_normal((N, data[k][1].size))) for k in INSTRUMENTS}
            if vname == "all" and N == 3:
                model["miri"][1, 2] = np.nan            # one sample whose model holds a NaN
            ns["MODEL"] = lambda *a, _m=model, **k: {key: v.copy() for key, v in _m.items()}
            cube_arg = cube[0] if N == 1 else cube
            out = ns["log_likelihood"](cube_arg, fp, config, None, {k: list(v) for k, v in data.items()}, None)
            assert np.shape(out) == (() if N == 1 else (N,))
            store["ll/%s/cube" % name] = cube
            for k in INSTRUMENTS:
                store["ll/%s/model/%s" % (name, k)] = model[k]
            store["ll/%s/out" % name] = np.asarray(out)
            cases.append({"name": name, "N": N, "present": list(present)})
    store["ll/cases"] = np.array(json.dumps(cases))
    out_path = os.path.join(HERE, "retrieve.npz")
    np.savez_compressed(out_path, **store)
    print("wrote %s (%d bytes, %d arrays)" % (out_path, os.path.getsize(out_path), len(store)))


if __name__ == "__main__":
    main()
