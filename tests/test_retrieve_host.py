"""``picaso_amd.retrieve`` on the host: the dictionary and prior functions and the likelihood against the reference's own
(tests/golden/retrieve.npz, tests/golden/make_retrieve.py: bit for bit), the pressure grid, the units the reference's sample
configuration uses, ``InstrumentsPlan``'s host tables and ``get_data``."""
import builtins
import copy
import json
import os
import shutil

import numpy as np
import pytest

from helpers import GOLDEN
from test_chemistry_host import DIR_1060, DIR_2121

Z = np.load(os.path.join(GOLDEN, "retrieve.npz"))
RETRIEVAL = json.loads(str(Z["config"]))
INSTRUMENTS = ("nirspec", "miri")


def test_prior_finder_finds_every_prior_in_order():
    from picaso_amd import retrieve as rt
    fitpars = rt.prior_finder(RETRIEVAL)
    assert list(fitpars.keys()) == json.loads(str(Z["prior_keys"]))
    assert not any(k.startswith("sampler") for k in fitpars) and "err_inf.nirspec" in fitpars
    assert fitpars["chemistry.free.H2O"] is RETRIEVAL["chemistry"]["free"]["H2O"]


def test_hypercube_rows_and_batch_have_the_references_bits():
    from picaso_amd import retrieve as rt
    fitpars = rt.prior_finder(RETRIEVAL)
    u, x = Z["cube/u"], Z["cube/x"]
    assert u.shape == (7, len(fitpars)) and np.all(u[0] == 0.5)
    for row, want in zip(u, x):
        got = rt.hypercube(row, fitpars)
        assert got.shape == want.shape and np.array_equal(got, want)
    batch = rt.hypercube(u, fitpars)
    assert batch.shape == x.shape and np.array_equal(batch, x)
    assert np.array_equal(rt.hypercube(list(u[3]), fitpars), x[3])
    bad = copy.deepcopy(RETRIEVAL)
    bad["offset"]["miri"]["prior"] = "cauchy"
    with pytest.raises(Exception) as err:
        rt.hypercube(u[0], rt.prior_finder(bad))
    assert str(err.value) == "Prior type not available"


def test_set_dict_value_and_find_values_for_key(capsys):
    from picaso_amd import retrieve as rt
    nested = {"a": {"b": {"value": 1.0, "unit": "bar"}, "c": 3}, "d": {"value": 2.0}}
    rows = json.loads(str(Z["setdict"]))
    assert len(rows) == 6 and [r[2] for r in rows] == [True, True, True, False, False, False]
    for path_string, value, returned, after in rows:
        data = copy.deepcopy(nested)
        assert rt.set_dict_value(data, path_string, value) is returned and data == after, path_string
    assert capsys.readouterr().out.count("set_dict_value:") == 3             # a note per refusal
    for data, key, want in json.loads(str(Z["findvalues"])):
        assert rt.find_values_for_key(data, key) == want, key


@pytest.mark.parametrize("case", json.loads(str(Z["ll/cases"])), ids=lambda c: c["name"])
def test_log_likelihood_is_the_references_number(case, monkeypatch):
    from picaso_amd import retrieve as rt
    name, N = case["name"], case["N"]
    retrieval = {k: v for k, v in RETRIEVAL.items() if k not in ("offset", "scaling", "err_inf") or k in case["present"]}
    config = {"InputOutput": {"observation_data": {k: "unused" for k in INSTRUMENTS}}, "retrieval": retrieval}
    data = {k: [Z["ll/data/%s/%s" % (k, c)] for c in "xye"] for k in INSTRUMENTS}
    assert [len(data[k][0]) for k in INSTRUMENTS] == [5, 3]
    model = {k: Z["ll/%s/model/%s" % (name, k)] for k in INSTRUMENTS}
    monkeypatch.setattr(rt, "MODEL", lambda *a, **k: {key: v.copy() for key, v in model.items()})
    cube, want = Z["ll/%s/cube" % name], Z["ll/%s/out" % name]
    keep = {k: [v.copy() for v in data[k]] for k in data}
    got = rt.log_likelihood(cube[0] if N == 1 else cube, rt.prior_finder(retrieval), config, None, data, None)
    assert np.shape(got) == (() if N == 1 else (N,)) and np.array_equal(got, want, equal_nan=True)
    assert all(np.array_equal(a, b) for k in data for a, b in zip(data[k], keep[k]))        # the data are not written to
    if name == "all_N3":
        assert list(np.isnan(got)) == [False, True, False]
    else:
        assert np.all(np.isfinite(got))


def test_pressure_grid_is_the_two_numpy_expressions():
    from picaso_amd import justdoit as jdi
    from picaso_amd import retrieve as rt
    cfg = dict(min=dict(value=1e-6, unit="bar"), max=dict(value=1e2, unit="bar"), nlevel=13, spacing="log")
    assert np.array_equal(rt.pressure_grid(cfg), np.logspace(np.log10(1e-6), np.log10(1e2), 13))
    lin = dict(cfg, spacing="linear")
    assert np.array_equal(rt.pressure_grid(lin), np.linspace(1e-6, 1e2, 13))
    pa = dict(min=dict(value=0.1, unit="Pa"), max=dict(value=3.0, unit="atm"), nlevel=7, spacing="log")
    assert np.array_equal(rt.pressure_grid(pa), np.logspace(np.log10(0.1 * 1e-5), np.log10(3.0 * 1.01325), 7))
    mbar = dict(min=dict(value=2.0, unit="mbar"), max=dict(value=5.0, unit="bar"), nlevel=4, spacing="linear")
    assert np.array_equal(rt.pressure_grid(mbar), np.linspace(2.0 * 1e-3, 5.0, 4))
    with pytest.raises(Exception, match="pressure unit 'furlong' not known"):
        rt.pressure_grid(dict(cfg, min=dict(value=1.0, unit="furlong")))
    # PT_handler lays the grid on the inputs object and the profile on the grid
    from picaso_amd.parameterizations import Parameterize
    case, p = jdi.inputs(calculation="browndwarf"), Parameterize()
    df = rt.PT_handler(dict(profile="isothermal", pressure=cfg, isothermal=dict(T=700.0)), case, p)
    assert case.nlevel == 13 and np.array_equal(np.asarray(df["pressure"]), rt.pressure_grid(cfg))
    assert np.all(np.asarray(df["temperature"]) == 700.0)


def test_units_of_the_sample_configuration_convert():
    from picaso_amd import justdoit as jdi
    assert jdi._to_cgs(10.0, "parsec", "distance") == 10.0 * 3.0856775814913674e18
    assert jdi._to_cgs(10.0, "pc", "distance") == jdi._to_cgs(10.0, "parsec", "distance")
    assert jdi._to_cgs(200.0, "AU", "separation") == 200.0 * 1.495978707e13
    assert jdi._to_cgs(90.0, "degree", "angle") == 90.0 * (np.pi / 180.0)
    assert jdi._to_cgs(0.3, "radian", "angle") == 0.3
    with pytest.raises(Exception, match="distance: unit 'furlong' not known; give a cgs value"):
        jdi._to_cgs(1.0, "furlong", "distance")


def test_refused_kinds_keep_their_own_messages():
    from picaso_amd import justdoit as jdi
    from picaso_amd import retrieve as rt
    from picaso_amd.parameterizations import Parameterize
    cfg = dict(min=dict(value=1e-4, unit="bar"), max=dict(value=10.0, unit="bar"), nlevel=6, spacing="log")
    for kind, word in (("madhu_seager_09_inversion", "astropy"), ("madhu_seager_09_noinversion", "astropy")):
        with pytest.raises(NotImplementedError, match=word):
            rt.PT_handler({"profile": kind, "pressure": cfg, kind: {}}, jdi.inputs(calculation="browndwarf"), Parameterize())
    p = Parameterize()
    case = jdi.inputs(calculation="browndwarf")
    case.add_pt(T=np.full(6, 500.0), P=rt.pressure_grid(cfg))
    p.add_class(case)
    with pytest.raises(NotImplementedError, match="virga"):
        rt._cloud_host("virga", {}, {}, p)


def test_visscher_chemistry_groups_rows_by_grid_file(tmp_path, monkeypatch):
    """The 1-D route on the synthetic grid directory: every case gets ``chem_interp_batch`` of its own file's table, one
    call per file for all the cases that select it (the device call is replaced by its numpy yardstick here)."""
    from picaso_amd import chemistry as ch
    from picaso_amd import justdoit as jdi
    from picaso_amd import retrieve as rt
    shutil.copytree(DIR_2121, str(tmp_path / "chemistry" / "visscher_grid_2121"))
    monkeypatch.setenv("picaso_refdata", str(tmp_path))
    calls = []

    def on_host(t, p, table, **kw):
        calls.append(t.shape)
        species, ab = ch.interp_numpy(t.ravel(), p.ravel(), table)
        return {s: ab[:, i].reshape(t.shape) for i, s in enumerate(species)}
    monkeypatch.setattr(ch, "chem_interp_batch", on_host)
    temps = np.unique(ch.read_visscher_2121(ch.select_visscher_2121(0.55, 0.0, DIR_2121))["temperature"])
    pres = np.logspace(-5, 1, 6)
    cases, params = [], []
    for k, (cto, mh) in enumerate(((0.55, 0.0), (0.27, 0.0), (0.6, 0.1))):
        c = jdi.inputs(calculation="browndwarf")
        c.add_pt(T=np.linspace(temps[0], temps[1], 6) + k, P=pres)
        cases.append(c)
        params.append(dict(cto_absolute={"value": cto} if k else cto, log_mh=mh))          # a fitted entry is {'value': v}
    rt._chem_visscher(cases, params)
    assert sorted(calls) == [(1, 6), (2, 6)]                             # rows 0 and 2 select the same file
    for c, kw in zip(cases, params):
        prof = c.inputs["atmosphere"]["profile"]
        mirror = jdi.inputs(calculation="browndwarf")
        mirror.add_pt(T=prof["temperature"], P=prof["pressure"])
        cto = kw["cto_absolute"]
        mirror.chem_interp(ch.visscher_2121(cto["value"] if isinstance(cto, dict) else cto, kw["log_mh"]))
        want = mirror.inputs["atmosphere"]["profile"]
        assert list(prof.keys()) == list(want.keys()) and len(prof.keys()) > 10
        assert all(np.array_equal(prof[k], want[k]) for k in want.keys())


def test_chemeq_visscher_1060_is_chem_interp_of_the_chosen_file(tmp_path, monkeypatch):
    from picaso_amd import chemistry as ch
    from picaso_amd import justdoit as jdi
    shutil.copytree(DIR_1060, str(tmp_path / "chemistry" / "visscher_grid_1060"))
    monkeypatch.setenv("picaso_refdata", str(tmp_path))
    temps = np.unique(ch.visscher_1060(1.0, 0.0)["temperature"])

    def case():
        c = jdi.inputs(calculation="browndwarf")
        c.add_pt(T=np.linspace(temps[0], temps[-1], 7), P=np.logspace(-5, 1, 7))
        return c
    got, want = case(), case()
    got.chemeq_visscher_1060(1.1, 0.05)                                  # the nearest file: c_o = 1.0, [M/H] = 0.0
    want.chem_interp(ch.visscher_1060(1.0, 0.0))
    a, b = got.inputs["atmosphere"]["profile"], want.inputs["atmosphere"]["profile"]
    assert list(a.keys()) == list(b.keys()) and "H2O" in a.keys() and all(np.array_equal(a[k], b[k]) for k in b.keys())
    # premix_atmosphere's 'visscher' branch reaches it without arguments: it says what is missing
    for call in (got.chemeq_visscher_1060, lambda: got.chemeq_visscher_1060(1.0)):
        with pytest.raises(NotImplementedError, match="needs c_o .* and log_mh"):
            call()
    clim = jdi.inputs(calculation="browndwarf")
    clim.inputs["approx"]["chem_method"] = "visscher_1060"
    clim.add_pt(T=np.full(7, 500.0), P=np.logspace(-5, 1, 7))
    with pytest.raises(NotImplementedError, match="c_o .* and log_mh"):
        clim.premix_atmosphere(None)
    with pytest.raises(Exception, match="Choose a C/O less than"):
        got.chemeq_visscher_1060(3.0, 0.0)


def test_instruments_plan_host_tables():
    from picaso_amd import justdoit as jdi
    from picaso_amd import regrid

    class Opa:
        wno = np.linspace(900.0, 4000.0, 700)
        nwno = 700
    opa = Opa()
    spec = {"g1": {"wl": np.array([3.0, 5.0, 4.0]), "R": 120.0}, "m1": {"newx": np.linspace(1000.0, 3800.0, 9)},
            "g2": {"wl": np.array([6.5, 2.8]), "R": np.array([80.0, 300.0])}, "m2": {"R": 60.0}}
    plan = jdi.instruments_plan(opa, spec)
    assert isinstance(plan, regrid.InstrumentsPlan) and isinstance(plan, regrid.Reduction)
    assert (plan.kind, plan.counts_key, plan.scale) == ("instruments", "instrument_counts", 1.0)
    members = {"g1": jdi.convolve_plan(opa, spec["g1"]["wl"], 120.0), "m1": jdi.regrid_plan(opa, newx=spec["m1"]["newx"]),
               "g2": jdi.convolve_plan(opa, spec["g2"]["wl"], spec["g2"]["R"]), "m2": jdi.regrid_plan(opa, R=60.0)}
    assert list(plan.slices) == list(spec) and plan.nout == sum(m.nout for m in members.values())
    n0 = 0
    for name, m in members.items():
        assert plan.members[name] is m                                   # the memoised member plans, unchanged
        s = plan.slices[name]
        assert (s.start, s.stop) == (n0, n0 + m.nout)
        n0 = s.stop
        assert np.array_equal(plan.out_wavenumber[s], m.out_wavenumber) and np.array_equal(plan.counts[s], m.counts)
        if m.kind == "convolve":
            assert all(np.array_equal(getattr(plan, k)[s], getattr(m, k)) for k in ("lo", "hi", "centre", "den"))
        else:
            assert np.array_equal(plan.lo[s], m.start[:-1]) and np.array_equal(plan.hi[s], m.start[1:])
    assert plan.lo.dtype == plan.hi.dtype == plan.col.dtype == np.int32
    # the device order: mean points first, col restores instrument order
    nmean = members["m1"].nout + members["m2"].nout
    assert (plan.nmean, plan.ngauss) == (nmean, 5) and sorted(plan.col) == list(range(plan.nout))
    is_mean = np.zeros(plan.nout, dtype=bool)
    is_mean[plan.slices["m1"]] = is_mean[plan.slices["m2"]] = True
    assert np.all(is_mean[plan.col[:nmean]]) and not np.any(is_mean[plan.col[nmean:]])
    assert np.all(np.diff(plan.col[:nmean]) > 0) and np.all(np.diff(plan.col[nmean:]) > 0)
    # by content: the same values give the same plan, a scale gives a sibling that shares the tables
    again = jdi.instruments_plan(opa, {k: {kk: np.array(vv) for kk, vv in v.items()} for k, v in spec.items()})
    assert again is plan
    scaled = jdi.instruments_plan(opa, spec, scale=2.5e-9)
    assert scaled is not plan and scaled.scale == 2.5e-9 and scaled.lo is plan.lo and scaled._dev is plan._dev
    assert jdi.instruments_plan(opa, spec, scale=2.5e-9) is scaled
    assert scaled in regrid._plans and scaled._siblings is plan._siblings      # destroy_context reaches the shared tables
    assert jdi.instruments_plan(opa, dict(reversed(list(spec.items())))) is not plan
    for bad in ({}, {"a": {"wl": [1.0]}}, {"a": [1.0, 2.0]}, [spec]):
        with pytest.raises(Exception, match="instrument"):
            jdi.instruments_plan(opa, bad)
    with pytest.raises(Exception, match="give one of them"):
        from picaso_amd import convolve
        convolve.reduction({"R": 50.0}, None, opa, spec)
    with pytest.raises(Exception, match="regrid= and convolve= are two ways"):
        convolve.reduction({"R": 50.0}, {"wl": [3.0], "R": 100.0}, opa)


def test_get_data_from_arrays_and_text_files(tmp_path, monkeypatch):
    from picaso_amd import retrieve as rt
    wl = np.array([5.0, 3.0, 4.0, 3.5])
    y, e, R = np.array([1.0, 2.0, 3.0, 4.0]), np.array([0.1, 0.2, 0.3, 0.4]), np.array([100.0, 200.0, 300.0, 400.0])
    np.savetxt(tmp_path / "three.txt", np.stack([wl, y, e], axis=1))
    np.savetxt(tmp_path / "four.txt", np.stack([wl, y, e, R], axis=1))
    config = {"observation_type": "thermal", "InputOutput": {"observation_data": {
        "arrays": {"wavelength": wl, "y": y, "e": e}, "arrays_R": {"wavelength": wl, "y": y, "e": e, "R": 150.0},
        "three": str(tmp_path / "three.txt"), "four": str(tmp_path / "four.txt")}}}
    data = rt.get_data(config)
    assert list(data) == ["arrays", "arrays_R", "three", "four"]                  # every instrument, not the last alone
    order = np.argsort(1e4 / wl)
    for key, n in (("arrays", 3), ("arrays_R", 4), ("three", 3), ("four", 4)):
        assert len(data[key]) == n
        assert np.array_equal(data[key][0], (1e4 / wl)[order]) and np.all(np.diff(data[key][0]) > 0)
        assert np.array_equal(data[key][1], y[order]) and np.array_equal(data[key][2], e[order])
    assert np.array_equal(data["four"][3], R[order]) and np.array_equal(data["arrays_R"][3], np.full(4, 150.0))
    spec = rt._instruments(config, data)
    assert set(spec["three"]) == {"newx"} and set(spec["four"]) == {"wl", "R"}
    assert np.array_equal(spec["four"]["wl"], 1e4 / data["four"][0])
    np.savetxt(tmp_path / "two.txt", np.stack([wl, y], axis=1))
    with pytest.raises(Exception, match="2 columns"):
        rt.get_data({"observation_type": "thermal", "InputOutput": {"observation_data": {"x": str(tmp_path / "two.txt")}}})
    real = builtins.__import__
    monkeypatch.setattr(builtins, "__import__",
                        lambda name, *a, **k: (_ for _ in ()).throw(ImportError(name)) if name == "xarray" else real(name, *a, **k))
    with pytest.raises(ImportError, match="xarray"):
        rt.get_data({"observation_type": "transmission", "InputOutput": {"observation_data": {"x": "spectrum.nc"}}})


def test_run_says_how_to_pass_a_configuration(monkeypatch):
    from picaso_amd import retrieve as rt
    with pytest.raises(Exception, match="Could not interpret"):
        rt.run()
    real = builtins.__import__
    monkeypatch.setattr(builtins, "__import__", lambda name, *a, **k: (_ for _ in ()).throw(ImportError(name))
                        if name in ("tomllib", "tomli") else real(name, *a, **k))
    with pytest.raises(ImportError, match="driver_dict"):
        rt.run(driver_file="driver.toml")
