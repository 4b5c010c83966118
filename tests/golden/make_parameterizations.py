"""Generate tests/golden/parameterizations.npz by running the REFERENCE's own parameterizations (build container only):

    python tests/golden/make_parameterizations.py

The reference's ``parameterizations`` module does not import here (astropy, virga), so the definitions are taken from its
files with ``ast`` and compiled at generation time next to numpy, scipy and pandas; none of their text is stored.  From
``picaso/parameterizations.py`` the module functions ``atlev``, ``picaso_format`` and ``cloud_averaging`` and the methods
``add_class``, ``deck_decay``, ``slab_decay``, ``cloud_brewster_grey``, ``cloud_hard_grey``, ``chem_free``, ``vmr_knots``,
``vmr_gradient``, ``pt_knots``, ``pt_zj24``, ``pt_guillot`` and ``pt_isothermal`` of ``Parameterize``, bound to a bare class;
from ``picaso/wavelength.py`` ``get_cld_input_grid``; from ``picaso/justdoit.py`` the method ``clouds`` of ``inputs`` (the
box clouds ``cloud_hard_grey`` goes through), bound to a bare class too.

The file holds inputs and outputs only:
  meta/numpy, meta/scipy      the versions that wrote it
  plevel/<nlayer>             pressure levels (bar) of the 3-, 5- and 12-layer grids;  tlevel/12 a temperature on the last
  grid/<nin>                  cloud wavenumber grids of 2, 7 and 67 points (two decimals: any reader parses them exactly)
                              and the 196 points of the reference's wave_EGP.dat, increasing (the reference's box
                              clouds, which cloud_hard_grey goes through, are written for 196 points and no other count)
  cases                       JSON: [{name, fn, nlayer, nin, kwargs, raises}], in the order they were run
  out/<name>/<column>         what the reference returned: the columns of a DataFrame, or ``value`` for an array
  avg/<name>/...              cloud_averaging: per deck k the record d<k>/opd_l, w0_l, g0_l, alpha, reference_wave, the deck's
                              own table d<k>/opd (cloud_brewster_grey's), and the averaged opd, w0, g0
"""
import ast
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

PLEVEL = {3: np.logspace(-4, 1, 4), 5: np.logspace(-5, 2, 6), 12: np.logspace(-6, 2, 13)}
GRIDS = {n: np.round(np.geomspace(45.0, 30000.0, n), 2) for n in (2, 7, 67)}
SHAPES = ((3, 2), (5, 7), (12, 67))

METHODS = ["add_class", "deck_decay", "slab_decay", "cloud_brewster_grey", "cloud_hard_grey", "chem_free", "vmr_knots",
           "vmr_gradient", "pt_knots", "pt_zj24", "pt_guillot", "pt_isothermal"]


def _reference():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pandas as pd
    import ref_shim
    from scipy import interpolate, special
    ns = {"np": np, "pd": pd, "os": os, "interpolate": interpolate, "special": special}

    def take(fname, names, cls=None):
        path = os.path.join(ref_shim.REF_ROOT, "picaso", fname)
        with open(path) as fh:
            body = ast.parse(fh.read(), path).body
        if cls is not None:
            body = [n for n in body if isinstance(n, ast.ClassDef) and n.name == cls][0].body
        nodes = [n for n in body if isinstance(n, ast.FunctionDef) and n.name in names]
        assert sorted(n.name for n in nodes) == sorted(names), (fname, names)
        exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)

    take("wavelength.py", ["get_cld_input_grid"])
    take("parameterizations.py", ["atlev", "picaso_format", "cloud_averaging"])
    take("parameterizations.py", METHODS, cls="Parameterize")
    Bare = type("Bare", (), {m: ns[m] for m in METHODS})
    take("justdoit.py", ["clouds"], cls="inputs")
    Inputs = type("Inputs", (), {"clouds": ns["clouds"]})
    return ns, Bare, Inputs, os.path.join(ref_shim.REF_ROOT, "reference")


def _grid_dir(grid):
    """A $picaso_refdata with ``grid`` as its wave_EGP.dat, decreasing as the reference's own file."""
    d = tempfile.mkdtemp()
    os.makedirs(os.path.join(d, "opacities"))
    with open(os.path.join(d, "opacities", "wave_EGP.dat"), "w") as fh:
        fh.write("   i   wavenumber\n")
        for i, w in enumerate(grid[::-1]):
            fh.write("%4d %.2f\n" % (i + 1, w))
    return d


def main():
    import pandas as pd
    import scipy
    ns, Bare, Inputs, refdata = _reference()
    store = {"meta/numpy": np.array(np.__version__), "meta/scipy": np.array(scipy.__version__)}
    ns["__refdata__"] = refdata
    grids = dict(GRIDS)
    grids[196] = ns["get_cld_input_grid"]()
    assert grids[196].size == 196 and np.array_equal(np.round(grids[196], 2), grids[196])
    dirs = {n: _grid_dir(g) for n, g in grids.items()}
    for n, g in grids.items():
        ns["__refdata__"] = dirs[n]
        assert np.array_equal(ns["get_cld_input_grid"](), g), n
        store["grid/%d" % n] = g
    tlevel = 900.0 * (PLEVEL[12] / 1e-2) ** 0.08 + 25.0 * np.cos(np.arange(13.0))
    store["tlevel/12"] = tlevel
    for n, p in PLEVEL.items():
        store["plevel/%d" % n] = p

    def param(nlayer, nin=2, temperature=False, gravity=None):
        case = Inputs()
        prof = {"pressure": PLEVEL[nlayer]}
        if temperature:
            prof["temperature"] = tlevel
        case.inputs = {"atmosphere": {"profile": pd.DataFrame(prof)}, "planet": {} if gravity is None else {"gravity": gravity},
                       "clouds": {}}
        case.nlevel = nlayer + 1
        ns["__refdata__"] = dirs[nin]
        p = Bare()
        p.add_class(case)
        return p

    cases = []

    def run(name, fn, nlayer, nin, kwargs, raises=False, **how):
        p = param(nlayer, nin, **how)
        rec = dict(name=name, fn=fn, nlayer=nlayer, nin=nin, kwargs=kwargs, raises=raises, how=how)
        cases.append(rec)
        if raises:
            try:
                getattr(p, fn)(**kwargs)
            except Exception as e:
                assert not isinstance(e, (TypeError, KeyError, AssertionError)), e
                return None
            raise AssertionError("%s did not raise" % name)
        out = getattr(p, fn)(**kwargs)
        if isinstance(out, pd.DataFrame):
            for c in out.columns:
                store["out/%s/%s" % (name, c)] = np.asarray(out[c].values, dtype=np.float64)
        else:
            store["out/%s/value" % name] = np.asarray(out, dtype=np.float64)
        return out

    # ---- cloud profile shapes, on every pressure grid
    decks = {3: ((-1.0, 0.005), (0.5, 1.0)), 5: ((-1.0, 0.005), (1.5, 1.0)), 12: ((-1.0, 0.005), (1.5, 1.0))}
    slabs = {3: ((-1.6, 1.8, 1.0), (-1.4, 1.5, 2.5)), 5: ((-3.0, 1.4, 1.0), (-3.0, 4.0, 0.3)),
             12: ((-2.3, 0.7, 1.0), (-4.3, 3.0, 2.5))}
    for nl in (3, 5, 12):
        capped = run("deck_cap_%d" % nl, "deck_decay", nl, 2, dict(ptop=decks[nl][0][0], dp=decks[nl][0][1]))
        assert capped[-1] == 100.0 and capped[0] != 100.0, capped
        free = run("deck_free_%d" % nl, "deck_decay", nl, 2, dict(ptop=decks[nl][1][0], dp=decks[nl][1][1]))
        assert not np.any(free == 100.0) and np.all(free > 0), free
        run("deck_default_dp_%d" % nl, "deck_decay", nl, 2, dict(ptop=0.0))
        near = run("slab_adjacent_%d" % nl, "slab_decay", nl, 2, dict(zip(("ptop", "dp", "reference_tau"), slabs[nl][0])))
        assert np.count_nonzero(near) == 2 and np.diff(np.nonzero(near)[0])[0] == 1, near
        wide = run("slab_wide_%d" % nl, "slab_decay", nl, 2, dict(zip(("ptop", "dp", "reference_tau"), slabs[nl][1])))
        assert np.count_nonzero(wide) >= min(3, nl - 1) and wide[0] == 0.0, wide
        run("slab_exception_%d" % nl, "slab_decay", nl, 2, dict(ptop=-2.3), raises=True)

    # ---- grey clouds
    brewster = {}
    for nl, nin in SHAPES:
        for i, (alpha, ref) in enumerate(((0, 1), (1.5, 1), (-0.7, 2.3), (0, 2.3))):
            for decay in ("deck", "slab"):
                kw = dict(decay_type=decay, alpha=alpha, ssa=0.3 + 0.2 * i, reference_wave=ref)
                if decay == "deck":
                    kw["deck_kwargs"] = dict(ptop=decks[nl][i % 2][0], dp=decks[nl][i % 2][1])
                else:
                    kw["slab_kwargs"] = dict(zip(("ptop", "dp", "reference_tau"), slabs[nl][i % 2]))
                name = "grey_%s_%d_%dx%d" % (decay, i, nl, nin)
                brewster[name] = (kw, run(name, "cloud_brewster_grey", nl, nin, kw))
    hard = run("hard_grey_5x196", "cloud_hard_grey", 5, 196, dict(g0=[0.8, -0.2], w0=[0.9, 0.5], opd=[2.0, 0.25],
                                                                p=[1.0, 0.0], dp=[4.0, 2.0]))
    per_layer = hard["opd"].values.reshape(5, 196)
    assert np.all(per_layer == per_layer[:, :1]) and set(per_layer[:, 0]) == {0.0, 2.0, 0.25}, per_layer[:, 0]
    assert list(per_layer[:, 0]).index(0.25) > list(per_layer[:, 0]).index(2.0)      # the second box lies inside the first
    run("hard_grey_int_5x196", "cloud_hard_grey", 5, 196, dict(g0=0, w0=1, opd=3, p=1, dp=2))

    # ---- cloud_averaging of 2 and 3 tables: decks with w0 and g0 per layer (g0 of mixed sign), nothing in the top layer
    rng = np.random.default_rng(20)
    for nl, nin in SHAPES[1:]:
        p = param(nl, nin)
        for tag, alphas in (("grey", (0, 0, 0)), ("colour", (1.5, -0.7, 0))):
            for K in (2, 3):
                name = "%s%d_%dx%d" % (tag, K, nl, nin)
                dfs = []
                for k in range(K):
                    ref = (1, 2.3, 0.8)[k]
                    if k == 1:
                        df = p.cloud_brewster_grey("deck", alphas[k], 0.5, reference_wave=ref,
                                                   deck_kwargs=dict(ptop=decks[nl][1][0], dp=decks[nl][1][1]))
                        df["opd"] = df["opd"].values * np.repeat(np.arange(nl) > 0, nin)          # nothing in the top layer
                    else:
                        df = p.cloud_brewster_grey("slab", alphas[k], 0.5, reference_wave=ref,
                                                   slab_kwargs=dict(zip(("ptop", "dp", "reference_tau"), slabs[nl][1 - k // 2])))
                    w0_l, g0_l = rng.uniform(0.1, 1.0, nl), rng.uniform(-0.9, 0.9, nl)
                    df["w0"], df["g0"] = np.repeat(w0_l, nin), np.repeat(g0_l, nin)
                    opd = df["opd"].values.reshape(nl, nin)
                    power = (1e4 / grids[nin] / ref) ** (-alphas[k])
                    # the layer vector the table was made from: the shape functions' own output
                    opd_l = (p.deck_decay(decks[nl][1][0], decks[nl][1][1]) * (np.arange(nl) > 0) if k == 1
                             else p.slab_decay(*slabs[nl][1 - k // 2]))
                    assert np.array_equal(opd, opd_l[:, None] * power[None, :])
                    pre = "avg/%s/d%d/" % (name, k)
                    store[pre + "opd_l"], store[pre + "w0_l"], store[pre + "g0_l"] = opd_l, w0_l, g0_l
                    store[pre + "alpha"], store[pre + "reference_wave"] = np.float64(alphas[k]), np.float64(ref)
                    store[pre + "opd"] = opd.copy()
                    dfs.append(df)
                assert not any(np.any(df["opd"].values.reshape(nl, nin)[0]) for df in dfs)
                out = ns["cloud_averaging"](dfs)
                for c in ("opd", "w0", "g0"):
                    store["avg/%s/%s" % (name, c)] = out[c].values.reshape(nl, nin).copy()
                assert np.all(store["avg/%s/opd" % name][0] == 1e-33) and np.all(store["avg/%s/opd" % name][1:] > 1e-33)

    # ---- chemistry (12 layers, with a temperature)
    knots = dict(profile="knots", P_knots={"P1": {"value": 1e-5}, "P2": {"value": 1e-2}, "P3": {"value": 10.0}},
                 vmr_knots={"v1": {"value": 1e-6}, "v2": {"value": 3e-4}, "v3": {"value": 2e-3}})
    knots_list = dict(profile="knots", P_knots=[1e-4, 1.0], vmr_knots={"a": {"value": 1e-3}, "b": {"value": 1e-5}})
    deep = dict(profile="gradient", bottom={"value": 1e-3}, p_switch={"value": 0.1}, gradient={"value": -0.8})
    top = dict(profile="gradient", top={"value": 2e-5}, p_switch={"value": 1e-3}, gradient={"value": 0.6})
    cap = dict(profile="gradient", top={"value": 0.2}, p_switch={"value": 1e-2}, gradient={"value": 1.5})
    run("chem_one_background", "chem_free", 12, 2, dict(H2O=dict(value=1e-4), CH4=knots, CO=deep,
                                                      background=dict(gases=["H2"])), temperature=True)
    run("chem_two_backgrounds", "chem_free", 12, 2, dict(H2O=dict(value=3e-3), NH3=top, CO2=knots_list,
                                                       background=dict(gases=["H2", "He"], fraction=5.667)), temperature=True)
    capped = run("chem_capped", "chem_free", 12, 2, dict(N2=cap), temperature=True)
    assert np.any(capped["N2"].values == 1.0) and np.any(capped["N2"].values < 1.0)
    run("vmr_gradient_deep", "vmr_gradient", 12, 2, dict(species=deep))
    run("vmr_gradient_top", "vmr_gradient", 12, 2, dict(species=top))
    run("vmr_knots", "vmr_knots", 12, 2, dict(species=knots))

    # ---- T(P)
    P4, T4 = [1e-1, 1e-5, 50.0, 1e-3], [900.0, 400.0, 2100.0, 650.0]                 # unsorted
    as_dict = lambda vals: {"k%d" % i: {"value": v} for i, v in enumerate(vals)}
    for nl in (5, 12):
        run("pt_brewster_%d" % nl, "pt_knots", nl, 2, dict(P_knots=P4, T_knots=T4, interpolation="brewster"))
        run("pt_linear_%d" % nl, "pt_knots", nl, 2, dict(P_knots=P4[:2], T_knots=T4[:2], interpolation="linear"))
        run("pt_quadratic_%d" % nl, "pt_knots", nl, 2, dict(P_knots=P4[:3], T_knots=T4[:3], interpolation="quadratic_spline"))
        run("pt_cubic_%d" % nl, "pt_knots", nl, 2, dict(P_knots=P4, T_knots=T4, interpolation="cubic_spline"))
        run("pt_cubic_dict_%d" % nl, "pt_knots", nl, 2, dict(P_knots=as_dict(P4), T_knots=as_dict(T4),
                                                            interpolation="cubic_spline"))
        run("pt_brewster_6_%d" % nl, "pt_knots", nl, 2, dict(P_knots=P4 + [3e-4, 4.0], T_knots=T4 + [500.0, 1500.0]))
        run("pt_zj24_%d" % nl, "pt_zj24", nl, 2, dict(pressures=[1e-4, 1e-2, 1.0, 60.0], dTs=[0.02, 0.08, 0.2, 0.27],
                                                      Tbottom={"value": 2400.0}))
        run("pt_zj24_dict_%d" % nl, "pt_zj24", nl, 2, dict(pressures=as_dict([1e-3, 1e-1, 10.0]), dTs=as_dict([0.05, 0.1, 0.25]),
                                                           Tbottom={"value": 1800.0}))
        run("pt_guillot_%d" % nl, "pt_guillot", nl, 2, dict(Teq=1200.0, T_int=150.0, logg1=-0.5, logKir=-1.5, alpha=0.4),
            gravity=2200.0)
        run("pt_isothermal_%d" % nl, "pt_isothermal", nl, 2, dict(T=777.0))

    # ---- picaso_format
    for nl, nin in SHAPES:
        p = param(nl, nin)
        opd, w0, g0 = rng.uniform(0.1, 3.0, nin), rng.uniform(0.2, 1.0, nin), rng.uniform(-0.5, 0.9, nin)
        decay = np.exp(-rng.uniform(0.0, 3.0, nl))
        forms = {"p_top": dict(p_top=float(p.pressure_layer[1]), p_bottom=float(p.pressure_layer[-1])),
                 "p_decay": dict(p_decay=decay, p_bottom=float(p.pressure_layer[-2])),
                 "opd_profile": dict(opd_profile=p.slab_decay(*slabs[nl][1]))}
        for tag, kw in forms.items():
            name = "format_%s_%dx%d" % (tag, nl, nin)
            out = ns["picaso_format"](opd, w0, g0, grids[nin], p.pressure_layer, **kw)
            for c in ("opd", "w0", "g0"):
                store["format/%s/in_%s" % (name, c)] = {"opd": opd, "w0": w0, "g0": g0}[c]
            for k, v in kw.items():
                store["format/%s/kw_%s" % (name, k)] = np.asarray(v, dtype=np.float64)
            for c in out.columns:
                store["format/%s/%s" % (name, c)] = np.asarray(out[c].values, dtype=np.float64)
            assert np.any(store["format/%s/opd" % name] == 0) and np.any(store["format/%s/opd" % name] > 0)

    store["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, "parameterizations.npz")
    np.savez_compressed(path, **store)
    size = os.path.getsize(path)
    print("wrote", path, "%.1f KB, %d cases" % (size / 1024, len(cases)))
    assert size <= 1024 * 1024, "a committed file holds 1 MiB"


if __name__ == "__main__":
    main()
